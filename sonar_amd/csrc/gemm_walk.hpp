// The persistent tile walk of the 256x256 GEMM engines (gemm.hip, gemm_v2.hip) and the block-id maps of every tiled kernel.
// Plain C++: compiles for the host too and includes no HIP header, so that a stand-alone program can replay the walk of every
// workgroup of a launch (tools/micro/gemm_route_walk.cpp).
#pragma once

#if defined(__HIP__)
#define SMI_WALK_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define SMI_WALK_FN inline
#endif

namespace smi {

// XCD-aware block id remap (bijective for any grid size): hardware deals
// block b to XCD b%8; give every XCD one contiguous range of logical ids so
// neighbouring tiles share that XCD's private L2.
SMI_WALK_FN int xcd_remap(int b, int nb) {
  const int q = nb >> 3, r = nb & 7;
  const int xcd = b & 7, idx = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// raster 0: XCD-aware grouped raster over 256x256 tiles in id order: the 32 workgroups resident on one XCD (1 per CU)
// cover an 8(m) x 4(n) super-tile, and with N/256 = 32 column tiles a persistent round is exactly one
// group, so an XCD keeps the SAME 4 W panels (2 MiB of its 4 MiB L2) round after round while the X
// panels stream through (measured against 4 x 8: FFN-inner 45.3 -> 44.7 ms per step).
SMI_WALK_FN void walk_grouped(int id, int ntm, int ntn, int& tile_m, int& tile_n) {
  constexpr int GM = 8;
  const int per_group = GM * ntn;
  const int group = id / per_group;
  const int first_m = group * GM;
  const int gsz = GM < ntm - first_m ? GM : ntm - first_m;
  const int in_group = id - group * per_group;
  tile_m = first_m + in_group % gsz;
  tile_n = in_group / gsz;
}

// raster 2 (full 256-workgroup grids, N >= 4 n-quads): XCD c OWNS the m-groups c, c + 8, ... (8 X panels each) and
// walks the n-quads of a group in consecutive rounds, in an order rotated by c.  With raster 0 and N = 8192 the
// 8 XCDs work on the SAME 8 X panels in every round (each on its own 4 W panels): every X panel is pulled across
// the fabric by all 8 XCDs at the same moment (PMC: 3.2 GB fetched per launch for 0.29 GB of operands).  With
// XCD-owned m-groups an X panel is fetched by one XCD only, and the rotation keeps the XCDs on different W panels.
// Measured (profiles/r02_experiments.txt, experiments 6-7): FFN inner 1.82-1.87 -> 1.75-1.76 ms
// (1175-1210 -> 1249-1260 TFLOP/s), 44.0 -> 41.9 ms per C2 step; no effect at N = 3072 (X is shared by 3 XCDs
// there), so it is used from 16 n tiles up.  (raster 1 = the same without the rotation.)
// Virtual ids t = 256 q + 32 c + j (round q, XCD c, slot j); the last m-group may be partial: its surplus slots,
// and XCDs that own one group fewer, skip the id (false).
// PARTS: the ids of raster 0 run over K parts of nout = ntm * ntn tiles each (walk_coords_parts below); else nout is unused.
template <bool PARTS>
SMI_WALK_FN bool walk_coords_of(int t, int raster, int ntm, int ntn, int nq, int& tile_m, int& tile_n, int nout) {
  if (raster == 0) {
    walk_grouped(PARTS ? t % nout : t, ntm, ntn, tile_m, tile_n);
    return true;
  }
  const int q = t / 256, c = (t % 256) / 32, j = t % 32;
  tile_m = (c + 8 * (q / nq)) * 8 + j % 8;
  tile_n = ((q + (raster == 2 ? c : 0)) % nq) * 4 + j / 8;
  return tile_m < ntm;
}
SMI_WALK_FN bool walk_coords(int t, int raster, int ntm, int ntn, int nq, int& tile_m, int& tile_n) {
  return walk_coords_of<false>(t, raster, ntm, ntn, nq, tile_m, tile_n, 0);
}
// The same over K parts (split-K of the 8-wave engine, which keeps the part index id / nout); rasters 1 and 2 have one part.
SMI_WALK_FN bool walk_coords_parts(int t, int raster, int ntm, int ntn, int nq, int nout, int& tile_m, int& tile_n) {
  return walk_coords_of<true>(t, raster, ntm, ntn, nq, tile_m, tile_n, nout);
}
// A workgroup walks the ids xcd_remap(block), + grid size, ... and skips the invalid ones:
//   while (t < nvirt && !walk_coords(t, ...)) t += gridDim.x;
// That loop stays a local lambda (`seek`) in each kernel: as a shared function hipcc renumbers the registers of every kernel
// that uses it (profiles/isa_identity.txt).

// number of virtual ids of rasters 1 and 2 (raster 0 walks the work units themselves)
SMI_WALK_FN int walk_nvirt(int ntm, int nq) { return ((ntm + 63) / 64) * nq * 256; }

}  // namespace smi
