// pm_workmap.h -- which (field pair, chunk) a workgroup of the pair scan kernels takes (pm_pair_scan, pm_pair_edit_scan).
// Plain C++ with no includes: the kernels and tests/test_pair_workmap.py's host harness compile the same functions.
//
// A grid has ncombos * nchunks workgroups, one per (combo, chunk); combo = field pair (the edit plan: test) and a
// combo's workgroups read one slot table (3 MiB at 200k patterns).  Both maps are bijections from blockIdx onto the
// (combo, chunk) items for any nchunks >= 1, ncombos >= 1; blockIdx >= ncombos * nchunks gets combo = ncombos (no item).
#pragma once

#if defined(__HIPCC__)
#define PM_HD __host__ __device__
#else
#define PM_HD
#endif

namespace pm {

constexpr int PAIR_XCDS = 8;                 // XCDs of an MI355X, blocks dealt round-robin: b and b + 8 run on one XCD (speed only)
enum { PAIR_MAP_SUPERCHUNK = 0, PAIR_MAP_XCD = 1, PAIR_MAP_XCD_SUPERCHUNK = 2 };

// Superchunks (the map up to round 4): runs of `group` chunks of one combo, all combos of a superchunk one after the
// other, the last superchunk shorter.  The superchunk's stream is re-read from MALL; but 256 CUs take a run of 256
// workgroups at once, and every CU that finishes takes its next workgroup from the next combo: the 32 CUs of an XCD
// almost always hold two combos, two 3 MiB tables in one 4 MiB L2.
PM_HD inline void pair_superchunk_item(int b, int nchunks, int ncombos, int group, int *combo, int *chunk) {
  if (b < 0 || b >= nchunks * ncombos) { *combo = ncombos; *chunk = nchunks; return; }
  const int per_super = group * ncombos;
  const int sc = b / per_super;
  const int rem = b - sc * per_super;
  int c = rem / group;
  int j = sc * group + (rem - c * group);
  const int full = (nchunks / group) * group;
  if (sc * group >= full) {
    const int tail = nchunks - full;
    const int r2 = b - (full / group) * per_super;
    c = r2 / tail;
    j = full + (r2 - c * tail);
  }
  *combo = c; *chunk = j;
}

// XCD-affine, combo-major: block b runs on XCD x = b % 8 as its (b / 8)-th workgroup.  The items in chunk-major order
// (i = chunk * ncombos + combo) are cut into 8 consecutive shares, XCD x's as large as its count of blocks; an XCD
// walks its share one combo after the other, chunks ascending.  So each XCD's 32 CUs work on ONE combo -- one slot
// table in its L2 -- except for the ~32 workgroups around a change of combo, and read their share of the stream once
// per combo (6 x 1/8 of the stream per XCD: from HBM at 3 Gbp, well inside its bandwidth).
PM_HD inline void pair_xcd_item(int b, int nchunks, int ncombos, int *combo, int *chunk) {
  if (b < 0 || b >= nchunks * ncombos) { *combo = ncombos; *chunk = nchunks; return; }
  const int G = nchunks * ncombos, q = G / PAIR_XCDS, r = G - q * PAIR_XCDS;
  const int x = b % PAIR_XCDS;
  int l = b / PAIR_XCDS;
  const int S = x * q + (x < r ? x : r);     // the share: items [S, E); blocks b < G with b % 8 == x: q + (x < r)
  const int E = S + q + (x < r ? 1 : 0);
  for (int c = 0; c < ncombos; ++c) {
    const int j0 = (S - c + ncombos - 1) / ncombos, j1 = (E - c + ncombos - 1) / ncombos;   // chunks j with S <= j ncombos + c < E
    if (l < j1 - j0) { *combo = c; *chunk = j0 + l; return; }
    l -= j1 - j0;
  }
  *combo = ncombos; *chunk = nchunks;
}

// XCD-contiguous shares of every superchunk: the superchunks and their combo-major item order as in
// pair_superchunk_item, but inside a superchunk XCD x takes ONE contiguous piece of that order, piece (x + superchunk)
// mod 8, as many items as the superchunk has blocks of XCD x.  At 6 combos and 256 chunks per superchunk a piece is 192
// items (6 per CU) of one or two combos, and the next superchunk's piece of the same XCD goes on where this one ends:
// an XCD walks the combo-major order without a jump, a change of combo every ~1.3 superchunks, and takes every piece
// in turn (combos that cost more -- the edit plan's tests -- are shared out over the XCDs).  The superchunk's stream is
// still read by all XCDs within the superchunk's time (its re-reads stay in MALL).
PM_HD inline void pair_xcd_superchunk_item(int b, int nchunks, int ncombos, int group, int *combo, int *chunk) {
  if (b < 0 || b >= nchunks * ncombos) { *combo = ncombos; *chunk = nchunks; return; }
  const int per_super = group * ncombos;
  const int sc = b / per_super;
  const int O = sc * per_super;                                  // first block = first item of the superchunk
  const int K = nchunks - sc * group < group ? nchunks - sc * group : group;   // its chunks (the last one is shorter)
  const int M = K * ncombos;
  const int R = O % PAIR_XCDS, x = b % PAIR_XCDS, rot = sc % PAIR_XCDS;
  const int p = (x + rot) % PAIR_XCDS;                           // XCD x takes piece p of this superchunk
  int S = 0;                                                     // items of the pieces in front of p: their XCDs' blocks in [O, O + M)
  for (int q = 0; q < p; ++q) {
    const int d = ((q - rot + PAIR_XCDS) % PAIR_XCDS - R + PAIR_XCDS) % PAIR_XCDS;
    if (d < M) S += (M - d + PAIR_XCDS - 1) / PAIR_XCDS;
  }
  const int t = S + (b - O) / PAIR_XCDS;                         // rank inside the superchunk, combo-major
  *combo = t / K; *chunk = sc * group + (t - (t / K) * K);
}

}  // namespace pm
