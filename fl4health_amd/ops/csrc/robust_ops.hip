// CDNA4 (gfx950) kernels for Byzantine-robust server aggregation.
//
// The K client rows arrive as SEPARATE fp32 buffers (no [K, n] stack is ever
// materialised): their pointers travel in a by-value kernel-argument struct.
// Same conventions as flat_ops.hip: 256-thread blocks, grid-stride loops
// capped at 8192 blocks, int64 indexing, one pass over HBM, no atomics, so
// both results are bitwise reproducible run to run.
//
//  rank_mean_rows      out[c] = mean of the ranks lo..hi-1 of column c
//                      (median, trimmed mean), NaN ordered last like
//                      torch.sort. Register-resident bitonic network.
//  pairwise_sqdist_rows D[i][j] = sum_c (x_i[c]-x_j[c])^2 from the differences
//                      (never the Gram form), fp32 runs of <= 64 terms folded
//                      into fp64, fixed partial slots + fixed-order finalize.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#define BLOCK 256
#define ROBUST_MAX_ROWS 64

static inline int grid_1d(int64_t n_items) {
  int64_t want = (n_items + BLOCK - 1) / BLOCK;
  int64_t cap = 8192;
  return (int)std::min(std::max<int64_t>(want, 1), cap);
}

#define GSL(i, n, stride) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (stride))
#define STRIDE ((int64_t)gridDim.x * blockDim.x)

struct RowPtrs {
  const float* p[ROBUST_MAX_ROWS];
};

// ---------------------------------------------------------------------------
// rank_mean_rows
// ---------------------------------------------------------------------------
// Order-preserving float -> uint32 key: -inf < finite < +inf < NaN (every NaN,
// either sign, maps to the top key, so pads and NaNs sort together above all
// real values). A compare-exchange is then one v_min_u32 + one v_max_u32;
// float min/max would drop NaNs.
__device__ __forceinline__ uint32_t f32_to_key(float x) {
  uint32_t b = __float_as_uint(x);
  uint32_t k = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
  return (x != x) ? 0xFFFFFFFFu : k;
}

__device__ __forceinline__ float key_to_f32(uint32_t k) {
  return __uint_as_float(k ^ ((uint32_t)((int32_t)(~k) >> 31) | 0x80000000u));
}

// Bitonic network; every index is a compile-time constant after unrolling so
// the array stays in VGPRs.
template <int P>
__device__ __forceinline__ void sort_network(uint32_t (&v)[P]) {
#pragma unroll
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int l = i ^ j;
        if (l > i) {
          uint32_t a = v[i], b = v[l];
          uint32_t mn = min(a, b), mx = max(a, b);
          if ((i & k) == 0) { v[i] = mn; v[l] = mx; } else { v[i] = mx; v[l] = mn; }
        }
      }
    }
  }
}

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float type; };
template <> struct VecOf<4> { typedef float4 type; };

// V adjacent columns starting at `col` (col % V == 0 and 4*V-byte aligned
// rows when V > 1). K > P/2 whenever P > 8, so the low half loads
// unconditionally; the rest sit behind a wave-uniform branch and pad with the
// NaN key.
template <int P, int V>
__device__ __forceinline__ void rank_mean_cols(const RowPtrs& rows, float* out, int K, int lo,
                                               int hi, int64_t col) {
  typedef typename VecOf<V>::type vec_t;
  uint32_t v[V][P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    if ((P > 8 && k < P / 2) || k < K) {
      vec_t x = *reinterpret_cast<const vec_t*>(rows.p[k] + col);
      const float* xs = reinterpret_cast<const float*>(&x);
#pragma unroll
      for (int c = 0; c < V; ++c) v[c][k] = f32_to_key(xs[c]);
    } else {
#pragma unroll
      for (int c = 0; c < V; ++c) v[c][k] = 0xFFFFFFFFu;
    }
  }
#pragma unroll
  for (int c = 0; c < V; ++c) sort_network<P>(v[c]);
  float acc[V];
#pragma unroll
  for (int c = 0; c < V; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int r = 0; r < P; ++r) {
    if (r >= lo && r < hi) {  // wave-uniform
#pragma unroll
      for (int c = 0; c < V; ++c) {
        float x = key_to_f32(v[c][r]);
        acc[c] = (r == lo) ? x : acc[c] + x;
      }
    }
  }
  const float cnt = (float)(hi - lo);
  vec_t o;
  float* os = reinterpret_cast<float*>(&o);
#pragma unroll
  for (int c = 0; c < V; ++c) os[c] = acc[c] / cnt;
  *reinterpret_cast<vec_t*>(out + col) = o;
}

template <int P, int V>
__global__ __launch_bounds__(BLOCK) void rank_mean_rows_kernel(RowPtrs rows, float* out, int K,
                                                               int lo, int hi, int64_t n) {
  const int64_t nv = n / V;
  GSL(g, nv, STRIDE) rank_mean_cols<P, V>(rows, out, K, lo, hi, g * V);
  if (V > 1) {
    GSL(t, n - nv * V, STRIDE) rank_mean_cols<P, 1>(rows, out, K, lo, hi, nv * V + t);
  }
}

template <int P, int V>
static void rank_mean_launch(const RowPtrs& rp, float* out, int K, int lo, int hi, int64_t n,
                             hipStream_t s) {
  rank_mean_rows_kernel<P, V><<<grid_1d(n / V + 1), BLOCK, 0, s>>>(rp, out, K, lo, hi, n);
}

// `aligned16`: every row pointer and `out` are 16-byte aligned. Only the small
// networks take four columns per thread: V*P <= 64 keys live per thread, and
// at P = 32 one column per thread (73 VGPRs) measured faster than two (141).
extern "C" void launch_rank_mean_rows(const float* const* rows, int K, float* out, int lo, int hi,
                                      int64_t n, int aligned16, hipStream_t s) {
  RowPtrs rp;
  for (int k = 0; k < ROBUST_MAX_ROWS; ++k) rp.p[k] = rows[k < K ? k : 0];
  if (K <= 8) {
    if (aligned16) rank_mean_launch<8, 4>(rp, out, K, lo, hi, n, s);
    else rank_mean_launch<8, 1>(rp, out, K, lo, hi, n, s);
  } else if (K <= 16) {
    if (aligned16) rank_mean_launch<16, 4>(rp, out, K, lo, hi, n, s);
    else rank_mean_launch<16, 1>(rp, out, K, lo, hi, n, s);
  } else if (K <= 32) {
    rank_mean_launch<32, 1>(rp, out, K, lo, hi, n, s);
  } else {
    rank_mean_launch<64, 1>(rp, out, K, lo, hi, n, s);
  }
}

// ---------------------------------------------------------------------------
// pairwise_sqdist_rows
// ---------------------------------------------------------------------------
// A block stages SQ_TC columns of all rows into LDS, transposed to
// tile[column][row] (row stride PK+4 floats: 16-byte aligned for b128 reads,
// skewed across banks for the transposing writes). Rows >= K and columns >= n
// are staged as zeros, which add exactly 0 to every pair.
// Each thread owns a 4x4 (i, j) sub-tile, SGEMM-style. (PK/4)^2 threads cover
// the PK x PK pairs; the 256/(PK/4)^2 thread groups ("slices") of a block take
// interleaved columns of the tile. fp32 runs are SQ_RUN terms long, then fold
// into the thread's fp64 accumulators. Slices are summed in fixed order
// through LDS, every block writes its K*K fp64 partials to its own slot, and
// the finalize kernel adds the slots in fixed order.
#define SQ_TC 64
#define SQ_RUN 64
#define SQ_SMEM_BYTES (BLOCK * 16 * 8)  // slice reduce: 256 threads x 16 doubles

static inline int sqdist_slots(int PK) { return PK <= 32 ? 2048 : 1024; }

template <int PK>
__global__ __launch_bounds__(BLOCK) void pairwise_sqdist_partial_kernel(
    RowPtrs rows, double* __restrict__ partial, int K, int64_t n) {
  constexpr int TD = PK / 4;              // threads per pair-tile side
  constexpr int TG = TD * TD;             // threads per slice
  constexpr int S = BLOCK / TG;           // slices
  constexpr int LDK = PK + 4;             // LDS row stride (floats)
  constexpr int EPT = PK * SQ_TC / BLOCK; // staged elements per thread
  constexpr int ITERS = SQ_TC / S;        // columns per thread per tile
  constexpr int FOLD_TILES = SQ_RUN / ITERS;
  static_assert(SQ_TC % S == 0 && SQ_RUN % ITERS == 0 && FOLD_TILES >= 1, "tile shape");
  static_assert(SQ_TC * LDK * 4 <= SQ_SMEM_BYTES, "tile must fit the shared buffer");

  __shared__ __align__(16) unsigned char smem[SQ_SMEM_BYTES];
  float* tile = reinterpret_cast<float*>(smem);
  double* red = reinterpret_cast<double*>(smem);

  const int tid = threadIdx.x;
  const int slice = tid / TG;
  const int ti = (tid % TG) / TD;
  const int tj = tid % TD;
  // staging role: element e = q*BLOCK + tid -> row e / SQ_TC, column e % SQ_TC
  const int sc = tid % SQ_TC;
  const int sk0 = tid / SQ_TC;  // rows sk0, sk0+4, ...

  const int64_t ntiles = (n + SQ_TC - 1) / SQ_TC;
  float stage[EPT];
  float acc[4][4];
  double dacc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) { acc[a][b] = 0.0f; dacc[a][b] = 0.0; }

  auto load_stage = [&](int64_t t) {
    const int64_t col = t * SQ_TC + sc;
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      const int k = sk0 + q * (BLOCK / SQ_TC);
      stage[q] = (k < K && col < n) ? rows.p[k][col] : 0.0f;
    }
  };

  int64_t t = blockIdx.x;
  if (t < ntiles) load_stage(t);
  int tiles_in_run = 0;
  for (; t < ntiles; t += gridDim.x) {
#pragma unroll
    for (int q = 0; q < EPT; ++q) tile[sc * LDK + sk0 + q * (BLOCK / SQ_TC)] = stage[q];
    __syncthreads();
    if (t + gridDim.x < ntiles) load_stage(t + gridDim.x);  // in flight during the math
#pragma unroll 4
    for (int c = slice; c < SQ_TC; c += S) {
      const float4 av = *reinterpret_cast<const float4*>(&tile[c * LDK + ti * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&tile[c * LDK + tj * 4]);
      const float a4[4] = {av.x, av.y, av.z, av.w};
      const float b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          float d = a4[a] - b4[b];
          acc[a][b] = fmaf(d, d, acc[a][b]);
        }
    }
    if (++tiles_in_run == FOLD_TILES) {
      tiles_in_run = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { dacc[a][b] += (double)acc[a][b]; acc[a][b] = 0.0f; }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) dacc[a][b] += (double)acc[a][b];

  // fixed-order sum over slices: red[slice][i][j]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      red[(slice * PK + ti * 4 + a) * PK + tj * 4 + b] = dacc[a][b];
  __syncthreads();
  double* dst = partial + (int64_t)blockIdx.x * K * K;
  for (int e = tid; e < K * K; e += BLOCK) {
    const int i = e / K, j = e % K;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += red[(s * PK + i) * PK + j];
    dst[e] = sum;
  }
}

// One block per (i, j): strided fp64 sums of the slots, fixed tree reduce.
__global__ __launch_bounds__(BLOCK) void pairwise_sqdist_final_kernel(
    const double* __restrict__ partial, double* __restrict__ out, int kk, int nslots) {
  __shared__ double sm[BLOCK];
  const int e = blockIdx.x;
  double acc = 0.0;
  for (int s = threadIdx.x; s < nslots; s += BLOCK) acc += partial[(int64_t)s * kk + e];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int off = BLOCK / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[e] = sm[0];
}

static inline int sqdist_padded(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64; }

// Number of partial slots ([slots, K, K] doubles) the launch below writes.
extern "C" int pairwise_sqdist_num_slots(int K, int64_t n) {
  int64_t ntiles = std::max<int64_t>((n + SQ_TC - 1) / SQ_TC, 1);
  return (int)std::min<int64_t>(ntiles, sqdist_slots(sqdist_padded(K)));
}

extern "C" void launch_pairwise_sqdist_rows(const float* const* rows, int K, double* partial,
                                            double* out, int64_t n, hipStream_t s) {
  RowPtrs rp;
  for (int k = 0; k < ROBUST_MAX_ROWS; ++k) rp.p[k] = rows[k < K ? k : 0];
  const int slots = pairwise_sqdist_num_slots(K, n);
  switch (sqdist_padded(K)) {
    case 8: pairwise_sqdist_partial_kernel<8><<<slots, BLOCK, 0, s>>>(rp, partial, K, n); break;
    case 16: pairwise_sqdist_partial_kernel<16><<<slots, BLOCK, 0, s>>>(rp, partial, K, n); break;
    case 32: pairwise_sqdist_partial_kernel<32><<<slots, BLOCK, 0, s>>>(rp, partial, K, n); break;
    default: pairwise_sqdist_partial_kernel<64><<<slots, BLOCK, 0, s>>>(rp, partial, K, n); break;
  }
  pairwise_sqdist_final_kernel<<<K * K, BLOCK, 0, s>>>(partial, out, K * K, slots);
}
