// Per-object colocalization (CellProfiler 4 MeasureColocalization object measurements, restated in
// include/cpx.h and DESIGN.md §12): for every object and every channel pair a < b the Pearson
// correlation, the overlap coefficient, both Manders coefficients and both K coefficients of the
// fp32 corrected planes widened to fp64.
//
// One 256-thread workgroup per object, two sweeps over the object's bbox:
//   sweep 1: n, sum x_a and max x_a per channel           -> mean_a, t_a = (thr / 100) * max_a
//   sweep 2: C centred squares, C (C - 1) / 2 centred products, C single-threshold sums and five
//            joint-threshold sums per pair (70 sums for C = 5), every one an fp64 register
//            accumulator of the thread (the kernel is a template on C, every loop unrolled).
// A thread visits the bbox pixels p = tid, tid + 256, ... in that order, a wave adds its lanes by
// the xor butterfly, the four waves' sums are added in wave order: the order of every sum depends
// on the bbox alone, so two runs give the same bits (no floating-point atomics anywhere).
#include "cpx_internal.h"

namespace {

constexpr int kColocThreads = 256;
constexpr int kColocWaves = kColocThreads / 64;

__host__ __device__ constexpr int coloc_pairs(int C) { return C * (C - 1) / 2; }
// index of the pair (a, b), a < b, in itertools.combinations(range(C), 2) order
__host__ __device__ constexpr int coloc_pair(int a, int b, int C) { return a * (2 * C - a - 1) / 2 + (b - a - 1); }
// sweep 2's sums, in the order they are reduced: [C] centred squares, [C] single-threshold sums,
// [NP] centred products, [NP][5] joint-threshold sums (x_a x_b, x_a^2, x_b^2, x_a, x_b)
__host__ __device__ constexpr int coloc_sums(int C) { return 2 * C + 6 * coloc_pairs(C); }

// np.max: the first NaN wins and stays
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int C>
__global__ __launch_bounds__(kColocThreads) void k_coloc(const int* __restrict__ labels,
                                                         const float* __restrict__ corr, int H, int W,
                                                         int max_label, const cpx_object* __restrict__ objects,
                                                         const cpx_fov_objects* __restrict__ hdr, double thr_pct,
                                                         double* __restrict__ out) {
  constexpr int NP = coloc_pairs(C), NS = coloc_sums(C);
  __shared__ double s_sum[kColocWaves][C];
  __shared__ float s_max[kColocWaves][C];
  __shared__ int s_n[kColocWaves];
  __shared__ double s_red[kColocWaves][NS];
  __shared__ double s_tot[NS];
  const int fov = blockIdx.y;
  const int n_obj = min(hdr[fov].n_objects, max_label);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long N = (long long)H * W;
  const int* lab = labels + (long long)fov * N;
  const float* img = corr + (long long)fov * C * N;
  for (int k = blockIdx.x; k < n_obj; k += gridDim.x) {
    const cpx_object o = objects[(long long)fov * max_label + k];
    const int L = o.label;
    // (a table row is trusted for its label, never for addresses: the bbox is cut to the plane)
    const int r0 = max(o.bbox[0], 0), c0 = max(o.bbox[1], 0);
    const int r1 = min(o.bbox[2], H), c1 = min(o.bbox[3], W);
    const int bw = max(c1 - c0, 0), bh = max(r1 - r0, 0);
    const long long nb = (long long)bh * bw;
    // the thread's pixels p = tid + i * 256 as (row, column) of the bbox, stepped without a division
    const int dr = bw ? kColocThreads / bw : 0, dc = bw ? kColocThreads % bw : 0;
    const int rr0 = bw ? (int)threadIdx.x / bw : 0, cc0 = bw ? (int)threadIdx.x % bw : 0;

    // ---- sweep 1 ---------------------------------------------------------------------------
    int n = 0;
    double s[C];
    float mx[C];
#pragma unroll
    for (int a = 0; a < C; ++a) {
      s[a] = 0.0;
      mx[a] = -INFINITY;
    }
    {
      int rr = rr0, cc = cc0;
      for (long long p = threadIdx.x; p < nb; p += kColocThreads) {
        const long long gi = (long long)(r0 + rr) * W + (c0 + cc);
        const int l = lab[gi];
        float v[C];
#pragma unroll
        for (int a = 0; a < C; ++a) v[a] = img[a * N + gi];
        if (l == L) {
          n += 1;
#pragma unroll
          for (int a = 0; a < C; ++a) {
            s[a] += (double)v[a];
            mx[a] = nan_max(mx[a], v[a]);
          }
        }
        rr += dr;
        cc += dc;
        if (cc >= bw) {
          cc -= bw;
          rr += 1;
        }
      }
    }
    n = wave_sum(n);
#pragma unroll
    for (int a = 0; a < C; ++a) {
      s[a] = wave_sum(s[a]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx[a] = nan_max(mx[a], __shfl_xor(mx[a], off, 64));
    }
    if (lane == 0) {
      s_n[wave] = n;
#pragma unroll
      for (int a = 0; a < C; ++a) {
        s_sum[wave][a] = s[a];
        s_max[wave][a] = mx[a];
      }
    }
    __syncthreads();
    n = 0;
#pragma unroll
    for (int w = 0; w < kColocWaves; ++w) n += s_n[w];
    double mean[C], t[C];
#pragma unroll
    for (int a = 0; a < C; ++a) {
      double sa = s_sum[0][a];
      float ma = s_max[0][a];
#pragma unroll
      for (int w = 1; w < kColocWaves; ++w) {
        sa += s_sum[w][a];
        ma = nan_max(ma, s_max[w][a]);
      }
      mean[a] = sa / (double)n;
      t[a] = (thr_pct / 100.0) * (double)ma;
    }

    // ---- sweep 2 ---------------------------------------------------------------------------
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    {
      int rr = rr0, cc = cc0;
      for (long long p = threadIdx.x; p < nb; p += kColocThreads) {
        const long long gi = (long long)(r0 + rr) * W + (c0 + cc);
        const int l = lab[gi];
        float v[C];
#pragma unroll
        for (int a = 0; a < C; ++a) v[a] = img[a * N + gi];
        if (l == L) {
          double x[C], d[C], xx[C];
          bool ge[C];
#pragma unroll
          for (int a = 0; a < C; ++a) {
            x[a] = (double)v[a];
            d[a] = x[a] - mean[a];
            xx[a] = x[a] * x[a];
            ge[a] = x[a] >= t[a];
            acc[a] += d[a] * d[a];
            acc[C + a] += ge[a] ? x[a] : 0.0;
          }
#pragma unroll
          for (int a = 0; a < C; ++a) {
#pragma unroll
            for (int b = a + 1; b < C; ++b) {
              const int pi = coloc_pair(a, b, C);
              const bool in = ge[a] && ge[b];
              acc[2 * C + pi] += d[a] * d[b];
              constexpr int kJ = 2 * C + NP;
              acc[kJ + 5 * pi + 0] += in ? x[a] * x[b] : 0.0;
              acc[kJ + 5 * pi + 1] += in ? xx[a] : 0.0;
              acc[kJ + 5 * pi + 2] += in ? xx[b] : 0.0;
              acc[kJ + 5 * pi + 3] += in ? x[a] : 0.0;
              acc[kJ + 5 * pi + 4] += in ? x[b] : 0.0;
            }
          }
        }
        rr += dr;
        cc += dc;
        if (cc >= bw) {
          cc -= bw;
          rr += 1;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const double r = wave_sum(acc[i]);
      if (lane == 0) s_red[wave][i] = r;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NS; i += kColocThreads) {
      double r = s_red[0][i];
#pragma unroll
      for (int w = 1; w < kColocWaves; ++w) r += s_red[w][i];
      s_tot[i] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < NP) {
      // thread pi -> its pair (a, b)
      int a = 0, rem = threadIdx.x;
      while (rem >= C - 1 - a) {
        rem -= C - 1 - a;
        a += 1;
      }
      const int b = a + 1 + rem, pi = threadIdx.x;
      const double* j = s_tot + 2 * C + NP + 5 * pi;
      double* q = out + ((long long)fov * max_label + k) * (CPX_N_COLOC * NP) + CPX_N_COLOC * pi;
      q[CPX_COLOC_CORRELATION] = s_tot[2 * C + pi] / sqrt(s_tot[a] * s_tot[b]);
      q[CPX_COLOC_OVERLAP] = j[0] / sqrt(j[1] * j[2]);
      q[CPX_COLOC_MANDERS_AB] = j[3] / s_tot[C + a];
      q[CPX_COLOC_MANDERS_BA] = j[4] / s_tot[C + b];
      q[CPX_COLOC_K_AB] = j[0] / j[1];
      q[CPX_COLOC_K_BA] = j[0] / j[2];
    }
    // (no barrier here: the next object's s_n / s_sum / s_max writes follow this object's last
    // barrier, which every thread passed after reading them; its s_red and s_tot writes follow
    // its own first barrier, which no thread reaches before it has read s_tot above)
  }
}

template <int C>
int launch(cpx_ctx* ctx, const int32_t* labels, const float* corr, int B, int H, int W, int max_label,
           const cpx_object* objects, const cpx_fov_objects* hdr, double thr, double* out) {
  // workgroups of a FOV stride over its objects; ~8 resident workgroups per CU over the batch
  const int per_fov = std::max(1, std::min(max_label, (8 * ctx->n_cu + B - 1) / B));
  hipLaunchKernelGGL(k_coloc<C>, dim3(per_fov, B), dim3(kColocThreads), 0, ctx->stream, (const int*)labels, corr,
                     H, W, max_label, objects, hdr, thr, out);
  CPX_CHECK_LAUNCH("k_coloc");
  return CPX_OK;
}

}  // namespace

extern "C" int cpx_n_colocalization(int C) { return C > 0 ? CPX_N_COLOC * coloc_pairs(C) : 0; }

extern "C" int cpx_colocalization(cpx_ctx* ctx, const int32_t* labels_dev, const float* corr_dev, int B, int C,
                                  int H, int W, int max_label, const cpx_object* objects_dev,
                                  const cpx_fov_objects* hdr_dev, double threshold_pct, double* coloc_dev) {
  CPX_REQUIRE(ctx, CPX_ERR_ARG, "cpx_colocalization: null context");
  CPX_REQUIRE(C >= 1 && C <= CPX_COLOC_MAX_CHANNELS, CPX_ERR_ARG,
              "cpx_colocalization: %d channels (1 .. %d supported)", C, CPX_COLOC_MAX_CHANNELS);
  CPX_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && max_label > 0, CPX_ERR_ARG,
              "cpx_colocalization: bad sizes");
  CPX_REQUIRE(threshold_pct >= 0.0 && threshold_pct <= 100.0, CPX_ERR_ARG,
              "cpx_colocalization: threshold_pct must be within 0 .. 100");
  if (C == 1) return CPX_OK;  // no pair, no column
  CPX_REQUIRE(labels_dev && corr_dev && objects_dev && hdr_dev && coloc_dev, CPX_ERR_ARG,
              "cpx_colocalization: null argument");
  switch (C) {
#define CPX_COLOC_CASE(c) \
  case c:                 \
    return launch<c>(ctx, labels_dev, corr_dev, B, H, W, max_label, objects_dev, hdr_dev, threshold_pct, coloc_dev);
    CPX_COLOC_CASE(2)
    CPX_COLOC_CASE(3)
    CPX_COLOC_CASE(4)
    CPX_COLOC_CASE(5)
    CPX_COLOC_CASE(6)
    CPX_COLOC_CASE(7)
    CPX_COLOC_CASE(8)
#undef CPX_COLOC_CASE
  }
  return CPX_ERR_ARG;
}
