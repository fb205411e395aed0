// Geometry of one implicit-GEMM launch, shared by the LDS-tiled kernels (igemm_nt.hip) and the wave-independent
// direct-fragment kernels (igemm_d16.hip).
#pragma once
#include "common.h"
#include <cstdio>

struct IgemmGeom {
  int mode;            // MMDYN_DENSE / MMDYN_CONV / MMDYN_TCONV_S2P1
  int G, Bg;           // groups, samples per group
  int Hr, Wr;          // row grid per sample (rows per sample = Hr*Wr)
  int Hi, Wi, Cin;     // gathered operand
  int Ho, Wo, N, ldc;  // output pixel grid, channels, row stride
  int rs, ro;          // input base of a row: y0 = r*rs + ro
  int os;              // output pixel of a row: (r*os + ph, c*os + pw)
  int ntaps, nclasses, splitk;
  int act, has_bias, want_stats, want_act_out;
  int rows_total;      // G*Bg*Hr*Wr (split-K workspace stride)
  int tiles_per_group; // ceil(Bg*Hr*Wr / BM); TCONV_S1P0: Ho*Wo*ceil(Bg/BM) (tiles never straddle an output pixel)
  int tiles_per_pixel; // TCONV_S1P0 only: ceil(Bg/BM)
  int s1p0_split;      // TCONV_S1P0 only: 1 = a block walks the four pixels of its quad, 2 = two blocks share the walk
  // optional BatchNorm+Swish backward epilogue (input-gradient launches): the tile of dL/d(activation) is turned
  // into du = da * swish'(gamma*xhat+beta) with xhat from the layer's saved pre-BN output, written to C, and the
  // per-tile column sums (du, du*xhat) go to `stats` -- the reduction pass of the BatchNorm backward disappears
  const float* bn_y;
  const float* bn_mean;   // [G][N]
  const float* bn_rstd;   // [G][N]
  const float* bn_gamma;  // [N]
  const float* bn_beta;   // [N]
  // bn_mean == nullptr with bn_y set: the plain ACTIVATION backward epilogue -- C = acc * act'(u), u = bn_y (the layer's
  // saved pre-activation at the C positions), act' chosen by bwd_act (MMDYN_ACT_SWISH / MMDYN_ACT_RELU); no statistics.
  // (with bn_mean set bwd_act is MMDYN_ACT_SWISH: the BatchNorm + Swish backward above)
  int bwd_act;
  // bf16 activation storage (bf16 matrix-core variants only): which of the activation tensors are bf16 in HBM
  int a_b16, c_b16, bny_b16;
  int cact_b16;   // the second (activated) output is bf16 while C itself is fp32
  int cact_planes;  // fp32x3 plane launches: the second (activated) output is a PLANE tensor, rows of [plane][cact_planes] bf16
                    // (cact_planes divides N, ldc == N); 0: a plain tensor
  int f16;     // the 16-bit format is IEEE half instead of bf16 (v_mfma_*_f16): operands, and every tensor the *_b16 fields mark
  int b_b16;   // packed weights are bf16 (written so by the pack kernels in the bf16 modes: half the L2 -> LDS traffic)
  // Grouped launch (mmdyn_igemm_nt_grouped): every group multiplies its OWN weights -- group grp reads Bp + grp * b_group_stride
  // and bias + grp * bias_group_stride (elements; 0 = one weight matrix shared by all groups, the BatchNorm-group form)
  int b_group_stride, bias_group_stride;
  int x3;          // fp32 launch on the bf16 matrix cores through the exact three-term operand split (igemm_nt.hip, X3)
  int tap_order;   // ring kernels, stride-2 CONV: the four taps of one input-pixel class back to back (0 = raster order)
  // persistent stream-K kernels (igemm_wsp.hip): arrival words of the split tiles, MMDYN_IGEMM_FLAG_WORDS zeroed uint32 the launch
  // leaves zero -- the tiles are then finished inside the launch; nullptr: slabs + the fix-up launch
  unsigned* flags;
};

// Shape -> row grid, output-parity classes and taps: the one place that knows the modes' geometry.  Fills the shape fields of *g
// for every mode and returns MMDYN_OK or the mode's shape error.  A launch returns that error; the host queries ignore it (they
// have always answered for any shape, and the launch is what refuses a bad one).
static inline int igemm_shape_geom(IgemmGeom* g, int mode, int G, int Bg, int Hi, int Wi, int Cin, int Ho, int Wo, int N, int ldc,
                                   int stride, int offset, int splitk) {
  g->mode = mode;
  g->G = G;
  g->Bg = Bg;
  g->Hi = Hi;
  g->Wi = Wi;
  g->Cin = Cin;
  g->Ho = Ho;
  g->Wo = Wo;
  g->N = N;
  g->ldc = ldc;
  g->splitk = splitk;
  g->Hr = Ho;
  g->Wr = Wo;
  g->rs = 1;
  g->ro = 0;
  g->os = 1;
  g->ntaps = 1;
  g->nclasses = 1;
  if (mode == MMDYN_DENSE) return (Hi != Ho || Wi != Wo) ? MMDYN_ERR_SHAPE : MMDYN_OK;
  if (mode == MMDYN_CONV) {
    g->rs = stride;
    g->ro = offset;
    g->ntaps = 16;
    return MMDYN_OK;
  }
  if (mode == MMDYN_IM2COL3) return (Hi != 2 * Ho || Wi != 2 * Wo || Cin != 64 || splitk != 1) ? MMDYN_ERR_SHAPE : MMDYN_OK;
  if (mode == MMDYN_TCONV_S1P0) {
    g->ntaps = 16;
    return (Ho != Hi + 3 || Wo != Wi + 3 || Ho != 8 || Wo != 8 || splitk != 1) ? MMDYN_ERR_SHAPE : MMDYN_OK;
  }
  if (mode == MMDYN_TCONV_S2P1) {
    g->Hr = Hi;
    g->Wr = Wi;
    g->os = 2;
    g->ntaps = 4;
    g->nclasses = 4;
    return (Ho != 2 * Hi || Wo != 2 * Wi) ? MMDYN_ERR_SHAPE : MMDYN_OK;
  }
  return MMDYN_ERR_SHAPE;
}

// BatchNorm partial-sum tiles per group of a launch that cuts its rows into M-tiles of bm: one per M-tile and parity class
// (TCONV_S1P0: per output pixel and sample tile -- a tile never straddles an output pixel)
static inline int igemm_m_tiles(const IgemmGeom& g, int bm) {
  if (g.mode == MMDYN_TCONV_S1P0) return g.Hr * g.Wr * ceil_div(g.Bg, bm);
  return g.nclasses * ceil_div(g.Bg * g.Hr * g.Wr, bm);
}

// ---- routing: the kernel family that serves a launch, and its plan (igemm_route in igemm_nt.hip is the one author) ----
enum IgemmFamily {
  IGEMM_NONE = 0,   // not served (only a plane launch can end here: every other one ends at the register-staged tiles)
  IGEMM_TILES,      // register-staged block tiles (igemm_nt.hip)
  IGEMM_TILES_X3,   // ... in the three-term split arithmetic
  IGEMM_WS,         // one-tile LDS-DMA ring (igemm_ws.hip)
  IGEMM_WSP,        // persistent stream-K ring (igemm_wsp.hip)
  IGEMM_WSP3,       // ... on operands that arrive split (the plane ring)
  IGEMM_PATCH,      // patch-resident k4 s2 p1 transposed convolution (tconv_patch.hip), fp32 or plane operands
  IGEMM_D16         // direct-fragment kernels (igemm_d16.hip, LAB build only)
};
// What a family's launcher branches on, decided once by its plan hook, and the two numbers the caller must know before the
// launch.  Fields a family does not use stay 0.
struct IgemmPlan {
  int family;
  int bm, bn;        // block tile (D16: the wave tile)
  int wm, wn;        // MFMA-wave tile, where one block tile is built with more than one (WSP, WSP3)
  int slots;         // LDS ring slots (WS, WSP, WSP3)
  int bpc;           // stream-K: resident blocks per CU the grid is sized for
  int per;           // stream-K: K-step units per block -- the cut of the schedule
  int x3;            // fp32 launch in the three-term split arithmetic
  int planes;        // PATCH: operands arrive split
  int stat_tiles;    // BatchNorm partial-sum tiles per group the launch writes into `stats`
  int slab_floats;   // floats of slab workspace the launch wants in `ws` (stream-K split tiles; 0: none)
};

// One hook pair per family.  plan: geometry (shape, splitk, storage flags, grouped weights, epilogue pointers) in; false = not
// served, else *p is filled.  launch: runs that plan and does not pick again; returns MMDYN_OK / an error code.
bool mmdyn_igemm_ws_plan(const IgemmGeom& g, bool bf16_ops, IgemmPlan* p);
int mmdyn_igemm_ws_launch(const float* A, const float* Bp, const float* bias, float* C, float* C_act, float* stats, float* ws,
                          const IgemmGeom& g, const IgemmPlan& p, bool bf16_ops, hipStream_t st);
bool mmdyn_igemm_wsp_plan(const IgemmGeom& g, bool bf16_ops, bool x3, IgemmPlan* p);
int mmdyn_igemm_wsp_launch(const float* A, const float* Bp, const float* bias, float* C, float* C_act, float* stats, float* slabs,
                           const IgemmGeom& g, const IgemmPlan& p, bool bf16_ops, hipStream_t st);
bool mmdyn_igemm_wsp3_plan(const IgemmGeom& g, IgemmPlan* p);
int mmdyn_igemm_wsp3_launch(const void* A, const void* Bp, const float* bias, float* C, float* C_act, float* stats, float* slabs,
                            const IgemmGeom& g, const IgemmPlan& p, hipStream_t st);
bool mmdyn_tconv_patch_plan(const IgemmGeom& g, bool planes, IgemmPlan* p);
int mmdyn_tconv_patch_launch(const void* A, const void* Bp, const float* bias, float* C, float* C_act, float* stats, float* ws,
                             const IgemmGeom& g, const IgemmPlan& p, hipStream_t st);
// LAB build only (igemm_d16.hip is not part of the product library: measured slower inside the two-lane step, LAB_NOTES A.a)
#ifdef MMDYN_LAB
bool mmdyn_igemm_d16_plan(const IgemmGeom& g, IgemmPlan* p);
int mmdyn_igemm_d16_launch(const float* A, const float* Bp, const float* bias, float* C, float* C_act, float* stats, float* ws,
                           const IgemmGeom& g, const IgemmPlan& p, hipStream_t st);
#else
static inline bool mmdyn_igemm_d16_plan(const IgemmGeom&, IgemmPlan*) { return false; }
#endif

// tile choice shared by the launcher and mmdyn_igemm_stat_tiles.  Measured on MI355X over every shape of the
// bs=256 step (tests/microbench/sweep_tiles.py): the 64x64 tile (more resident blocks per CU to hide the
// single-stage fetch latency) wins or ties everywhere except long-K problems that still fill the chip with
// 128x128 tiles; N == 32 (mod 64) takes 128x32.
// (rows_per_group, G) describe the row segments a tile may not straddle: groups, or (group, output pixel) pairs
static inline void pick_tile(int N, int rows_per_group, int G, int ncls, int splitk, int ksteps, int* bm, int* bn) {
  if (N % 64) {
    *bm = 128;
    *bn = 32;
  } else {
    *bm = 64;
    *bn = 64;
    if (N % 128 == 0 && splitk == 1 && ksteps >= 32 &&
        (long)G * ceil_div(rows_per_group, 128) * (N / 128) * ncls >= 512) {
      *bm = 128;
      *bn = 128;
    }
  }
  if (const char* ov = lab_env("MMDYN_IGEMM_TILE")) {   // kernel experiments only
    int a = 0, b = 0;
    if (sscanf(ov, "%d,%d", &a, &b) == 2 && N % b == 0) {
      *bm = a;
      *bn = b;
    }
  }
}

