// Opt-in Haralick texture columns (definitions in include/cpx.h and DESIGN.md §14): per object,
// channel and direction the nine Haralick features the Texture_* block lacks (Variance,
// SumAverage, SumVariance, SumEntropy, Entropy, DifferenceVariance, DifferenceEntropy, InfoMeas1,
// InfoMeas2) of the same 256-level, non-symmetric count matrix N the six greycoprops columns
// are computed from (k_texture.hip / k_features.hip, which this file leaves alone).
//
// One 1024-thread workgroup per (object, channel) item, one workgroup per CU (all of the LDS):
//   range   one sweep over the bbox: min / max of the masked crop (members' values, and 0 if the
//           bbox holds a non-member), as k_obj_stage has it
//   stage   a crop of up to kHarCrop pixels is quantised once into LDS as u8; a larger one is
//           quantised again from the plane and the labels wherever a pixel is needed
//   then per direction (T = the number of pairs, known from the bbox alone)
//   count   one integer LDS atomic per pair on the 128 KiB pair table: 65536 packed u16 counters
//           while T <= 65535 (no counter can pass T), else 128 rows of u32 counters in two passes
//           (reference levels 0..127, then 128..255), so no count is ever lost; a byte flag per
//           reference level marks the rows that hold anything
//   scan    wave w takes rows w, w + 16, ..., flagged rows only (one ballot over its flags); a
//           lane reads its four cells of the row and clears them; the non-zero cells are packed
//           across the wave (forward permute, lane order within a step), so that 64 cells at a
//           time add c (log2 T - log2 c) to their lane's entropy sum and c to nx[i], ny[j],
//           nsum[i + j], ndiff[|i - j|] (integer LDS atomics): a matrix has ~1,000 non-zero
//           cells in ~20,000 scanned ones
//   hist    thread t takes word t of nx | ny | ndiff | nsum (a wave holds one kind), threads
//           0..255 also word 1024 + t (the rest of nsum), and clears them: the entropy term and
//           k n, k^2 n; wave sums by the xor butterfly go to LDS, per direction
//   finish  after the four directions, lane 0 of wave d adds direction d's wave sums in wave
//           order and writes the nine columns
// Entropies: H(q) = -sum q log2 q with q = n / T is evaluated as (1 / T) sum n (log2 T - log2 n):
// every term is >= 0 (no cancellation), and a histogram with one occupied bin gives exactly +0.0.
// log2 n comes from a 256-entry LDS table the workgroup fills with log2() itself, or from log2()
// for larger n: the same value either way.
// Variances: (T sum k^2 n - (sum k n)^2) / T^2 with the numerator an exact integer while it fits
// 64 bits (T <= kHarExactT, which covers a full 2080 x 2080 plane), in float64 beyond.
// Every float64 sum runs in an order fixed by the bbox and the counts alone; the atomics are
// integer: two runs give the same bits.
#include "cpx_internal.h"

namespace {

constexpr int kHT = 1024;
constexpr int kHW = kHT / 64;
constexpr int kHarTab = 32768;        // u32 words of the pair table (128 KiB)
constexpr int kHarCrop = 21504;       // u8 crop pixels held in LDS (146 x 147)
constexpr long long kHarExactT = 8000000;  // 510^2 T^2 < 2^64 up to here
constexpr int kHx = 0, kHy = 256, kHd = 512, kHs = 768, kHistWords = 1280;  // nx, ny, ndiff, nsum[511] (+ 1)
constexpr int kLogTab = 256;

struct HarShared {
  unsigned int tab[kHarTab];
  unsigned int hist[kHistWords];  // nx, ny, ndiff, nsum
  double l2[kLogTab];             // log2 n, n < 256 (l2[0] unused)
  // a direction's wave sums: [0] the scan's cells, [1] the wave's words t, [2] its words 1024 + t
  double red_d[4][kHW][3];
  unsigned long long red_i[4][kHW][4];  // sum k n, sum k^2 n of the words t; of the words 1024 + t
  unsigned char flag[256];
  float sf[3][kHW];
  unsigned char crop[kHarCrop];
};
static_assert(sizeof(HarShared) <= 160 * 1024, "k_texture_haralick: LDS");

// scale_to_8bit of one pixel of the masked crop: k_texture.hip's quantize(), kept identical (the
// cross-block identity test, Contrast = DifferenceVariance + Dissimilarity^2, catches drift)
__device__ __forceinline__ int har_quantize(float v, bool in, float mn, float rng, bool flat) {
  const float m = v * (in ? 1.0f : 0.0f);
  if (flat) return 0;
  float x = m - mn;  // scale_to_8bit: 255.0 * (x - min) / (max - min), fp32, truncation
  x = 255.0f * x;
  x = x / rng;
  return (int)(unsigned char)(int)x;
}

// n (log2 T - log2 n), n > 0: T times the term of bin n in H = -sum (n / T) log2 (n / T); 0 for n == T
__device__ __forceinline__ double har_ent(const HarShared& s, unsigned int n, double lT) {
  const double l = n < (unsigned int)kLogTab ? s.l2[n] : log2((double)n);
  return (double)n * (lT - l);
}

// (T s2 - s1^2) / T^2: the variance of a histogram with sum n = T, sum k n = s1, sum k^2 n = s2
__device__ __forceinline__ double har_var(long long T, unsigned long long s1, unsigned long long s2) {
  const double Td = (double)T;
  if (T <= kHarExactT) return (double)((unsigned long long)T * s2 - s1 * s1) / (Td * Td);
  const double mu = (double)s1 / Td;
  return fmax((double)s2 / Td - mu * mu, 0.0);
}

// skimage graycomatrix offsets at distance 3: (0, 3), (2, 2), (3, 0), (2, -2)
__device__ __forceinline__ int har_dr(int d) { return d == 0 ? 0 : (d == 2 ? 3 : 2); }
__device__ __forceinline__ int har_dc(int d) { return d == 0 ? 3 : (d == 1 ? 2 : (d == 2 ? 0 : -2)); }

__global__ __launch_bounds__(kHT) void k_texture_haralick(const int* __restrict__ labels,
                                                          const float* __restrict__ corr, int C, int H, int W,
                                                          int max_label, const cpx_object* __restrict__ objects,
                                                          const cpx_fov_objects* __restrict__ hdr,
                                                          double* __restrict__ out) {
  __shared__ HarShared s;
  const int fov = blockIdx.y;
  const int n_obj = min(hdr[fov].n_objects, max_label);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long N = (long long)H * W;
  const int* lab = labels + (long long)fov * N;
  for (int x = threadIdx.x; x < kHarTab; x += kHT) s.tab[x] = 0u;
  for (int x = threadIdx.x; x < kHistWords; x += kHT) s.hist[x] = 0u;
  if (threadIdx.x < 256) {
    s.flag[threadIdx.x] = 0;
    s.l2[threadIdx.x] = log2((double)max((int)threadIdx.x, 1));
  }
  __syncthreads();
  const long long n_items = (long long)n_obj * C;
  for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int k = (int)(item / C), ch = (int)(item - (long long)k * C);
    const cpx_object ob = objects[(long long)fov * max_label + k];
    const float* img = corr + ((long long)fov * C + ch) * N;
    double* row = out + ((long long)fov * max_label + k) * ((long long)4 * CPX_N_HAR * C) + 4 * CPX_N_HAR * ch;
    const int L = ob.label;
    // (a table row is trusted for its label, never for addresses: the bbox is cut to the plane)
    const int r0 = max(ob.bbox[0], 0), c0 = max(ob.bbox[1], 0);
    const int bh = max(min(ob.bbox[2], H) - r0, 0), bw = max(min(ob.bbox[3], W) - c0, 0);
    const int nb = bh * bw;  // <= H * W < 2^31
    if (nb <= 0) {
      if (threadIdx.x < 4 * CPX_N_HAR) row[threadIdx.x] = 0.0;
      continue;
    }
    const long long org = (long long)r0 * W + c0;
    // ---- range of the masked crop ---------------------------------------------------------------
    float mn = INFINITY, mx = -INFINITY;
    bool nm = false;
    {
      int rr = (int)threadIdx.x / bw, cc = (int)threadIdx.x % bw;
      const int dr = kHT / bw, dc = kHT % bw;
#pragma unroll 1
      for (int p = threadIdx.x; p < nb; p += kHT) {
        const long long a = org + (long long)rr * W + cc;
        if (lab[a] == L) {
          const float v = img[a];
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
        } else {
          nm = true;
        }
        rr += dr;
        cc += dc;
        if (cc >= bw) {
          cc -= bw;
          rr += 1;
        }
      }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    const bool wnm = __builtin_amdgcn_ballot_w64(nm) != 0ull;
    if (lane == 0) {
      s.sf[0][wave] = mn;
      s.sf[1][wave] = mx;
      s.sf[2][wave] = wnm ? 1.0f : 0.0f;
    }
    __syncthreads();
    mn = s.sf[0][0];
    mx = s.sf[1][0];
    float anm = s.sf[2][0];
#pragma unroll
    for (int w = 1; w < kHW; ++w) {
      mn = fminf(mn, s.sf[0][w]);
      mx = fmaxf(mx, s.sf[1][w]);
      anm = fmaxf(anm, s.sf[2][w]);
    }
    if (anm != 0.0f) {  // the bbox holds a non-member: its 0 is in the crop
      mn = fminf(mn, 0.0f);
      mx = fmaxf(mx, 0.0f);
    }
    const float rng = mx - mn;
    const bool flat = !(mx != mn);
    // ---- the crop as u8 in LDS, when it fits ----------------------------------------------------
    const bool staged = nb <= kHarCrop;
    if (staged) {
      int rr = (int)threadIdx.x / bw, cc = (int)threadIdx.x % bw;
      const int dr = kHT / bw, dc = kHT % bw;
#pragma unroll 1
      for (int p = threadIdx.x; p < nb; p += kHT) {
        const long long a = org + (long long)rr * W + cc;
        s.crop[p] = (unsigned char)har_quantize(img[a], lab[a] == L, mn, rng, flat);
        rr += dr;
        cc += dc;
        if (cc >= bw) {
          cc -= bw;
          rr += 1;
        }
      }
    }
    __syncthreads();  // (the crop is complete; sf is free for the next item)
    auto level = [&](int rr, int cc) -> int {
      if (staged) return s.crop[rr * bw + cc];
      const long long a = org + (long long)rr * W + cc;
      return har_quantize(img[a], lab[a] == L, mn, rng, flat);
    };
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
      const int dr = har_dr(d), dc = har_dc(d);
      const int Th = bh - dr, Tw = bw - (dc < 0 ? -dc : dc);
      if (Th <= 0 || Tw <= 0) {  // no pair: nine +0.0
        if (threadIdx.x < CPX_N_HAR) row[CPX_N_HAR * d + threadIdx.x] = 0.0;
        continue;
      }
      const int T = Th * Tw;  // reference pixels: rows 0 .. Th - 1, columns cs .. cs + Tw - 1
      const int cs = dc < 0 ? -dc : 0;
      const bool wide = T > 65535;
      const double lT = log2((double)T);
      double exy = 0.0;  // the lane's cells: sum c (log2 T - log2 c)
      for (int half = 0; half < (wide ? 2 : 1); ++half) {
        // ---- count ------------------------------------------------------------------------------
        {
          int rr = (int)threadIdx.x / Tw, cc = (int)threadIdx.x % Tw;
          const int sr = kHT / Tw, sc = kHT % Tw;
#pragma unroll 1
          for (int t = threadIdx.x; t < T; t += kHT) {
            const int i = level(rr, cs + cc), j = level(rr + dr, cs + cc + dc);
            if (!wide) {
              atomicAdd(&s.tab[(i * 256 + j) >> 1], 1u << (16 * (j & 1)));
              s.flag[i] = 1;
            } else if ((i >> 7) == half) {
              atomicAdd(&s.tab[(i & 127) * 256 + j], 1u);
              s.flag[i] = 1;
            }
            rr += sr;
            cc += sc;
            if (cc >= Tw) {
              cc -= Tw;
              rr += 1;
            }
          }
        }
        __syncthreads();
        // ---- scan: the wave's flagged rows, four cells of a row per lane, in column order -------
        const int base = wide ? half * 128 : 0, nper = wide ? 128 / kHW : 256 / kHW;
        unsigned int queue = 0u;  // (16-bit passes) the lane's queued cell, i << 24 | j << 16 | c, or 0
        int fill = 0;             // queued cells (lanes 0 .. fill - 1), the same in every lane
        auto cell = [&](int i, int j, unsigned int c) {
          exy += har_ent(s, c, lT);
          atomicAdd(&s.hist[kHx + i], c);
          atomicAdd(&s.hist[kHy + j], c);
          atomicAdd(&s.hist[kHs + i + j], c);
          atomicAdd(&s.hist[kHd + (i > j ? i - j : j - i)], c);
        };
        auto flush = [&]() {
          if (lane < fill) cell((int)(queue >> 24), (int)((queue >> 16) & 255u), queue & 0xFFFFu);
          queue = 0u;
          fill = 0;
        };
        unsigned long long rows = __builtin_amdgcn_ballot_w64(lane < nper && s.flag[base + wave + kHW * lane] != 0);
        while (rows) {
          const int r = wave + kHW * (__ffsll((long long)rows) - 1);
          rows &= rows - 1ull;
          const int i = base + r;
          unsigned int c0v, c1v, c2v, c3v;
          int jlo;  // the lane's columns: jlo, jlo + 1, jlo + 128, jlo + 129 (packed) or lane + 64 u
          if (!wide) {  // words lane and lane + 64 of the row's 128
            unsigned int* p = &s.tab[r * 128 + lane];
            const unsigned int v0 = p[0], v1 = p[64];
            if (v0) p[0] = 0u;
            if (v1) p[64] = 0u;
            c0v = v0 & 0xFFFFu;
            c1v = v0 >> 16;
            c2v = v1 & 0xFFFFu;
            c3v = v1 >> 16;
            jlo = 2 * lane;
          } else {
            unsigned int* p = &s.tab[r * 256 + lane];
            c0v = p[0];
            c1v = p[64];
            c2v = p[128];
            c3v = p[192];
            if (c0v) p[0] = 0u;
            if (c1v) p[64] = 0u;
            if (c2v) p[128] = 0u;
            if (c3v) p[192] = 0u;
            jlo = lane;
          }
          if (!wide) {
            // the row's non-zero cells join the wave's queue: one packed cell (i, j, c) per lane, so
            // that the entropy terms and the histogram adds run on full lanes.  A forward permute
            // moves them: the cells of this step go to lanes fill .. fill + cnt - 1 in lane order,
            // the other lanes send 0 to the remaining lanes (a full permutation; OR keeps the queue)
#pragma unroll 1
            for (int u = 0; u < 4; ++u) {
              const unsigned int c = u == 0 ? c0v : (u == 1 ? c1v : (u == 2 ? c2v : c3v));
              const unsigned long long m = __builtin_amdgcn_ballot_w64(c != 0u);
              if (!m) continue;
              const int cnt = __popcll(m);
              if (fill + cnt > 64) flush();
              const int j = jlo + (u & 1) + 64 * (u & 2);
              const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
              const int dst = c ? fill + rank : (fill + cnt + lane - rank) & 63;
              const unsigned int val = c ? ((unsigned int)i << 24 | (unsigned int)j << 16 | c) : 0u;
              queue |= (unsigned int)__builtin_amdgcn_ds_permute(dst << 2, (int)val);
              fill += cnt;
            }
          } else if (c0v | c1v | c2v | c3v) {
#pragma unroll 1
            for (int u = 0; u < 4; ++u) {
              const unsigned int c = u == 0 ? c0v : (u == 1 ? c1v : (u == 2 ? c2v : c3v));
              if (c) cell(i, jlo + 64 * u, c);
            }
          }
          if (lane == 0) s.flag[i] = 0;
        }
        flush();
        __syncthreads();
      }
      // ---- the 1-D histograms: word t (nx | ny | ndiff | nsum by wave), then word 1024 + t -------
      double ea = 0.0, eb = 0.0;
      unsigned long long s1a = 0ull, s2a = 0ull, s1b = 0ull, s2b = 0ull;
#pragma unroll 1
      for (int part = 0; part < (wave < 4 ? 2 : 1); ++part) {
        const int x = (int)threadIdx.x + 1024 * part;
        const unsigned int n = s.hist[x];
        if (n) {
          s.hist[x] = 0u;
          const unsigned int kk = x < kHs ? (unsigned int)(x & 255) : (unsigned int)(x - kHs);
          const double e = har_ent(s, n, lT);
          const unsigned long long s1 = (unsigned long long)kk * n, s2 = (unsigned long long)(kk * kk) * n;
          ea = part == 0 ? e : ea;
          s1a = part == 0 ? s1 : s1a;
          s2a = part == 0 ? s2 : s2a;
          eb = part == 1 ? e : eb;
          s1b = part == 1 ? s1 : s1b;
          s2b = part == 1 ? s2 : s2b;
        }
      }
      exy = wave_sum(exy);
      ea = wave_sum(ea);
      s1a = wave_sum(s1a);
      s2a = wave_sum(s2a);
      if (wave < 4) {
        eb = wave_sum(eb);
        s1b = wave_sum(s1b);
        s2b = wave_sum(s2b);
      }
      if (lane == 0) {
        s.red_d[d][wave][0] = exy;
        s.red_d[d][wave][1] = ea;
        s.red_d[d][wave][2] = eb;
        s.red_i[d][wave][0] = s1a;
        s.red_i[d][wave][1] = s2a;
        s.red_i[d][wave][2] = s1b;
        s.red_i[d][wave][3] = s2b;
      }
    }
    __syncthreads();  // (the four directions' wave sums are in LDS; the crop is free)
    // ---- finish: lane 0 of wave d adds direction d's wave sums in wave order --------------------
    if (wave < 4 && lane == 0) {
      const int d = wave;
      const int Th = bh - har_dr(d), Tw = bw - (har_dc(d) < 0 ? -har_dc(d) : har_dc(d));
      if (Th > 0 && Tw > 0) {
        const int T = Th * Tw;
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                   // T times HXY, HX, HY, Hdiff, Hsum
        unsigned long long m[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};  // sum k n, sum k^2 n of nx, ndiff, nsum
#pragma unroll 1
        for (int w = 0; w < kHW; ++w) e[0] += s.red_d[d][w][0];
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {  // the kinds' four waves each, in wave order
          e[1] += s.red_d[d][w][1];
          e[2] += s.red_d[d][4 + w][1];
          e[3] += s.red_d[d][8 + w][1];
          e[4] += s.red_d[d][12 + w][1];
          m[0] += s.red_i[d][w][0];
          m[1] += s.red_i[d][w][1];
          m[2] += s.red_i[d][8 + w][0];
          m[3] += s.red_i[d][8 + w][1];
          m[4] += s.red_i[d][12 + w][0];
          m[5] += s.red_i[d][12 + w][1];
        }
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {  // nsum's words 1024 .. 1279
          e[4] += s.red_d[d][w][2];
          m[4] += s.red_i[d][w][2];
          m[5] += s.red_i[d][w][3];
        }
        const double Td = (double)T;
        const double hxy = e[0] / Td, hx = e[1] / Td, hy = e[2] / Td;
        const double hmax = fmax(hx, hy);
        double* q = row + CPX_N_HAR * d;
        q[CPX_HAR_VARIANCE] = har_var(T, m[0], m[1]);
        q[CPX_HAR_SUM_AVERAGE] = (double)m[4] / Td;
        q[CPX_HAR_SUM_VARIANCE] = har_var(T, m[4], m[5]);
        q[CPX_HAR_SUM_ENTROPY] = e[4] / Td;
        q[CPX_HAR_ENTROPY] = hxy;
        q[CPX_HAR_DIFFERENCE_VARIANCE] = har_var(T, m[2], m[3]);
        q[CPX_HAR_DIFFERENCE_ENTROPY] = e[3] / Td;
        q[CPX_HAR_INFO_MEAS1] = hmax > 0.0 ? (hxy - hx - hy) / hmax : 0.0;
        q[CPX_HAR_INFO_MEAS2] = sqrt(fmax(0.0, 1.0 - exp(-2.0 * (hx + hy - hxy))));
      }
    }
    // (the next item's wave sums are written two barriers from here: its range and stage barriers)
  }
}

}  // namespace

extern "C" int cpx_n_texture_haralick(int C) { return C > 0 ? 4 * CPX_N_HAR * C : 0; }

extern "C" int cpx_texture_haralick(cpx_ctx* ctx, const int32_t* labels_dev, const float* corr_dev, int B, int C,
                                    int H, int W, int max_label, const cpx_object* objects_dev,
                                    const cpx_fov_objects* hdr_dev, double* out_dev) {
  CPX_REQUIRE(ctx, CPX_ERR_ARG, "cpx_texture_haralick: null context");
  CPX_REQUIRE(C >= 1, CPX_ERR_ARG, "cpx_texture_haralick: %d channels (at least 1)", C);
  CPX_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && max_label > 0 && (long long)H * W < (1ll << 31),
              CPX_ERR_ARG, "cpx_texture_haralick: bad sizes");
  CPX_REQUIRE(labels_dev && corr_dev && objects_dev && hdr_dev && out_dev, CPX_ERR_ARG,
              "cpx_texture_haralick: null argument");
  // workgroups of a FOV stride over its (object, channel) items; one is resident per CU (LDS),
  // four per CU over the batch even out the items' sizes
  const long long items = (long long)max_label * C;
  const int per_fov = (int)std::max(1ll, std::min(items, (long long)(4 * ctx->n_cu + B - 1) / B));
  hipLaunchKernelGGL(k_texture_haralick, dim3(per_fov, B), dim3(kHT), 0, ctx->stream, (const int*)labels_dev,
                     corr_dev, C, H, W, max_label, objects_dev, hdr_dev, out_dev);
  CPX_CHECK_LAUNCH("k_texture_haralick");
  return CPX_OK;
}
