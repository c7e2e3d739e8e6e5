// Block -> (expert, row tile) mapping of the grouped expert GEMM
// (grouped_gemm.hip).  ONE function, compiled for the device (every block
// calls it on its row-tile index) and for the host (the grouped_gemm_plan
// binding runs it over a CPU offsets tensor so tests can check the mapping
// without a launch).
//
// offs is the (E+1,) row-offset table of a token buffer sorted by expert:
// expert e owns rows [offs[e], offs[e+1]).  Every offset is clamped to
// [0, T] before anything is derived from it and offs[e+1] <= offs[e] is an
// empty segment, so whatever the table holds, a tile lies inside [0, T).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_HD __host__ __device__ __forceinline__
#else
#define GG_HD inline
#endif

constexpr int GG_BM = 256;  // rows per tile of the fprop / dgrad kernels

struct GGTile {
  int expert;  // -1: idle block (beyond the last row tile)
  int row0;    // first row of the tile in the token buffer
  int rows;    // 1..GG_BM rows of the tile that belong to the segment
};

template <typename OffT>
GG_HD long gg_clamped(const OffT* offs, int i, long T) {
  const long v = (long)offs[i];
  return v < 0 ? 0 : (v > T ? T : v);
}

// Launch bound on the number of row tiles from host-known values only:
// sum_e ceil(c_e / BM) <= floor(T / BM) + E (each non-empty segment adds at
// most one partial tile), and never more than T (a tile holds >= 1 row).
GG_HD long gg_row_tile_bound(long T, int E) {
  const long b = T / GG_BM + E;
  return b < T ? b : T;
}

// The rt-th row tile, counting the tiles of expert 0, then 1, ...
template <typename OffT>
GG_HD GGTile gg_find_tile(const OffT* offs, int E, long T, long rt) {
  long first = 0;  // index of the current expert's first tile
  for (int e = 0; e < E; ++e) {
    const long lo = gg_clamped(offs, e, T);
    const long hi = gg_clamped(offs, e + 1, T);
    const long c = hi > lo ? hi - lo : 0;
    const long nt = (c + GG_BM - 1) / GG_BM;
    if (rt < first + nt) {
      const long r0 = lo + (rt - first) * GG_BM;
      const long left = hi - r0;
      return GGTile{e, (int)r0, (int)(left < GG_BM ? left : GG_BM)};
    }
    first += nt;
  }
  return GGTile{-1, 0, 0};
}
