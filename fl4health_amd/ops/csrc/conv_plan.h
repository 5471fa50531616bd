// Launch contract of the direct 3x3 conv kernels (conv_ops.hip): the LDS
// capacities the kernels size their __shared__ arrays from, and conv_plan(),
// the one place that derives tile geometry / grid and decides whether a shape
// fits a kernel. Plain C++17 (no HIP, no torch) so the kernels, the bindings
// and host-only checks all read the same numbers.
#pragma once
#include <cstdint>
#include <cstring>

constexpr int CONV_CB = 64;        // reduction channels per LDS stage (128-B rows)
constexpr int CONV_KB = 64;        // output channels per block, base/glds kernels
constexpr int CONVC_KB = 32;       // output channels per weight slab, kb32/kzloop
constexpr int CONV_THREADS = 256;  // 4-wave block
constexpr int CONV_GRID_CAP = 256; // persistent-weight glds grid cap (~CU count)

// Input-halo capacities. A halo position is CONV_CB bf16 = 8 chunks of 16 B.
// glds issues whole 64-lane groups, so a staged halo occupies its chunk count
// ROUNDED UP to 64; conv_plan compares the rounded count against the cap.
constexpr int CONV_TILE_POS = 304;          // base: positions (W=32: 6*34=204; W=4 SB=8: 288)
constexpr int CONV_GLDS_CHUNK_CAP = 1792;   // glds<4>, per buffer (32x32 M=128: 1632)
constexpr int CONV_GLDS_CHUNK_CAP8 = 2752;  // glds<8>, per buffer (32x32 M=256: 2720)
constexpr int CONVC_CHUNK_CAP = 2304;       // kb32, per buffer (4x4 SB=8: 288 pos * 8)
constexpr int CONVC_WCHUNKS = 9 * CONVC_KB * CONV_CB / 8;  // chunks per kb32/kzloop weight slab
// kzloop: the plan admits halos up to CONVD_IN_CHUNKS (16x16: 1440 -> 1472,
// 8x8 SB=2: 1600); the buffer keeps one glds group of slack on top of that.
constexpr int CONVD_IN_CHUNKS = 1600;
constexpr int CONVD_IN_CAP = CONVD_IN_CHUNKS + 64;  // chunks per resident input c-chunk
constexpr int CONVD_MAX_CC = 2;                     // resident input c-chunks (C <= 128)

// wrw (dW): deterministic split count, stage-1 combine groups, and the
// channel x filter slice one launch covers (workspaces are sized from these).
constexpr int WRW_SPLITS = 256;
constexpr int WRW_SG = 16;
constexpr int WRW_SLICE = 64;

// CONV_FWD is not a kernel: it asks conv_plan to pick among glds8, glds4 and
// base for the conv3x3_fwd entry point.
enum ConvKernel { CONV_BASE, CONV_GLDS4, CONV_GLDS8, CONV_KB32, CONV_KZLOOP, CONV_FWD };

struct ConvKernelSpec {
  const char* name;
  int waves;      // block = waves * 64 threads
  int m_rows;     // output positions per tile (the waves covering M, x 32)
  int kb;         // output channels per grid.z step (0: the block loops all K)
  int chunk_cap;  // rounded input chunks admitted per buffer
  int c_align, c_max, k_align;
  int grid_cap;   // grid.x = min(n_tiles, grid_cap); 0 = one block per tile
};

constexpr ConvKernelSpec CONV_SPECS[] = {
    {"base", 4, 128, CONV_KB, CONV_TILE_POS * (CONV_CB / 8), 1, INT32_MAX, 1, 0},
    {"glds4", 4, 128, CONV_KB, CONV_GLDS_CHUNK_CAP, 8, CONV_CB, 1, 2 * CONV_GRID_CAP},
    {"glds8", 8, 256, CONV_KB, CONV_GLDS_CHUNK_CAP8, 8, CONV_CB, 1, CONV_GRID_CAP},
    {"kb32", 4, 128, CONVC_KB, CONVC_CHUNK_CAP, CONV_CB, INT32_MAX, CONVC_KB, 0},
    // 8 waves, but wave pairs split K: 4 waves x 32 rows cover M
    {"kzloop", 8, 128, 0, CONVD_IN_CHUNKS, CONV_CB, CONVD_MAX_CC * CONV_CB, CONVC_KB, 0},
};

struct ConvPlan {
  ConvKernel kernel;
  int N, H, W, C, K;
  int BH, SB;  // image rows / packed samples per tile
  int h_groups, n_tiles;
  int waves, m_rows;
  int grid_x, grid_z;
  int64_t in_chunks;  // 16-B input chunks per buffer, rounded up to 64
  bool fits;
  const char* reason;  // "" when fits
};

inline const char* conv_kernel_name(ConvKernel k) { return k == CONV_FWD ? "fwd" : CONV_SPECS[k].name; }

// Returns false for an unknown name.
inline bool conv_kernel_from_name(const char* name, ConvKernel* out) {
  for (int k = CONV_BASE; k <= CONV_FWD; ++k)
    if (std::strcmp(name, conv_kernel_name((ConvKernel)k)) == 0) {
      *out = (ConvKernel)k;
      return true;
    }
  return false;
}

inline ConvPlan conv_plan(ConvKernel kernel, int N, int H, int W, int C, int K) {
  if (kernel == CONV_FWD) {
    // preference order: 8-wave glds (2 waves/SIMD), 4-wave glds, base
    ConvPlan p = conv_plan(CONV_GLDS8, N, H, W, C, K);
    if (!p.fits) p = conv_plan(CONV_GLDS4, N, H, W, C, K);
    if (!p.fits) p = conv_plan(CONV_BASE, N, H, W, C, K);
    return p;
  }
  const ConvKernelSpec& s = CONV_SPECS[kernel];
  ConvPlan p = {};
  p.kernel = kernel;
  p.N = N, p.H = H, p.W = W, p.C = C, p.K = K;
  p.waves = s.waves;
  p.m_rows = s.m_rows;
  p.reason = "";
  if (N < 1 || H < 1 || W < 1 || C < 1 || K < 1) {
    p.reason = "empty shape";
    return p;
  }
  // M = SB*BH*W output positions: BH image rows of one sample, or SB whole
  // small images packed into one tile
  int64_t hw = (int64_t)H * W;
  p.BH = s.m_rows / W < 1 ? 1 : (s.m_rows / W > H ? H : s.m_rows / W);
  int64_t sb = s.m_rows / hw < 1 ? 1 : s.m_rows / hw;
  p.SB = (int)(sb > N ? N : sb);
  int64_t h_groups = ((int64_t)H + p.BH - 1) / p.BH;
  int64_t n_tiles = (((int64_t)N + p.SB - 1) / p.SB) * h_groups;
  int64_t chunks = (int64_t)p.SB * (p.BH + 2) * ((int64_t)W + 2) * (CONV_CB / 8);
  p.in_chunks = (chunks + 63) & ~(int64_t)63;
  int64_t grid_z = s.kb ? ((int64_t)K + s.kb - 1) / s.kb : 1;
  if (C % s.c_align != 0 || K % s.k_align != 0)
    p.reason = "channel counts not a multiple of the kernel's C/K step";
  else if (C > s.c_max)
    p.reason = "C exceeds the channels the kernel keeps in LDS";
  else if ((int64_t)p.SB * p.BH * W > s.m_rows)
    p.reason = "image row wider than the M tile";
  else if (p.in_chunks > s.chunk_cap)
    p.reason = "input halo exceeds the LDS buffer";
  else if (n_tiles > INT32_MAX || grid_z > 65535)
    p.reason = "grid too large";
  if (p.reason[0] != '\0') return p;
  p.h_groups = (int)h_groups;
  p.n_tiles = (int)n_tiles;
  p.grid_x = s.grid_cap && p.n_tiles > s.grid_cap ? s.grid_cap : p.n_tiles;
  p.grid_z = (int)grid_z;
  p.fits = true;
  return p;
}
