"""Writes tests/golden/wild_long_parent.txt: for every handle of tests/test_gpu_wild_long.py's golden_cases() -- lists (a)-(g),
k = 0 / -K 1 / -K 2, pm_config.long_patterns = 32 and 127 -- the describe() text after one whole scan, the number of hits
and a digest of them -- one tab-separated line per handle: key, hits, digest, text -- as a build of the commit BEFORE PM_WILD_LONG existed gives them.  Needs a GPU.

Build that commit's library as a variant inside csrc/ (make VARIANT=_parent in a checkout of it, copy libpm_gpu_parent.so
over) and run
    PM_GPU_LIB=sequence-alignment-tools_amd/csrc/libpm_gpu_parent.so PM_GPU_LIB_AB=1 python tests/golden/make_wild_long_parent.py [out.txt]
The values 32 and 127 mean the same to that library as to this one; the test then asks this build for the same texts."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_gpu_wild_long as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wild_long_parent.txt")
    c = T.case()
    codes, table, _ = c["streams"]["table"]
    gold = {}
    for key, lst, name, bits in T.golden_cases():
        _, d, got = T.run(c["lists"][lst], name, codes, table, bits=bits)
        assert got == T.want_of(lst, name, "table"), key              # (the parent's hits are the oracle's)
        gold[key] = "%s\t%d\t%s\t%s\n" % (key, len(got), T.digest(got), d)
    with open(out, "w") as f:
        f.write("".join(gold[key] for key in sorted(gold)))
    print("wrote %d handles to %s" % (len(gold), out))


if __name__ == "__main__":
    main()
