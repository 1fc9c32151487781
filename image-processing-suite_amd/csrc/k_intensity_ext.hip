// Per-object intensity quantile, edge and location columns (the part of CellProfiler 4's
// MeasureObjectIntensity beyond Integrated / Mean / Std / Min / Max; definitions in include/cpx.h
// and DESIGN.md §13): quartiles, median and MAD by exact rank selection, the five statistics of
// the object's edge pixels, centre of mass, mass displacement and the place of the maximum.
//
// One 384-thread workgroup per object (blockIdx.y = FOV, the FOV's workgroups stride over its
// object table).  Per object:
//   geometry  one sweep over the bbox: the object's pixels are compacted by ballot, in raster
//             order, into LDS as (bbox-local index | edge bit << 31) while n <= CPX_IEXT_LDS_PIXELS;
//             n, |E|, sum r and sum c are integer sums.
//   then per channel
//   sums      sum x, sum r x, sum c x, (max, first place), and over E: sum x, min, max; the
//             channel's values go to LDS as monotone u32 keys (NaN on top, -0.0 as +0.0)
//   edge var  sum_E (x - mean_E)^2
//   select    4 radix passes of 8 bits find the (at most six) ranks the three quantiles need at
//             once: a 256-bin LDS histogram per distinct prefix, integer LDS atomics only
//   MAD       8 radix passes over the u64 pattern of |x - median| (a float64, computed from the
//             key on the fly), two ranks
// An object of more than CPX_IEXT_LDS_PIXELS pixels takes the same passes over its bbox in
// global memory (label and edge tests repeated, values served by L2); no workspace either way.
// Sums: a thread adds its elements (LDS path: compacted pixels i = tid, tid + 384, ...; bbox path:
// bbox pixels p = tid, tid + 384, ...) in that order, a wave adds its lanes by the xor butterfly,
// the six waves' sums are added in wave order: the order depends on the bbox and the pixel set
// alone, so two runs give the same bits.
#include "cpx_internal.h"

namespace {

constexpr int kIxThreads = 384;
constexpr int kIxWaves = kIxThreads / 64;
constexpr int kIxLds = CPX_IEXT_LDS_PIXELS;
constexpr int kIxTargets = 6;  // ranks i and i + 1 of the three quantiles
constexpr uint32_t kNanKey = 0xFFFFFFFFu;
constexpr uint32_t kEdgeBit = 0x80000000u;

// fp32 -> u32 key, ascending as numpy.sort orders the values: NaN last, -0.0 == +0.0
__device__ __forceinline__ uint32_t ix_key(float x) {
  if (x != x) return kNanKey;
  const uint32_t b = x == 0.0f ? 0u : __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ix_val(uint32_t k) {
  if (k == kNanKey) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// a float64 >= 0 or NaN -> u64 key
__device__ __forceinline__ unsigned long long ix_dkey(double w) {
  return w != w ? ~0ull : (unsigned long long)__double_as_longlong(w);
}
__device__ __forceinline__ double ix_dval(unsigned long long k) {
  return k == ~0ull ? (double)__uint_as_float(0x7FC00000u) : __longlong_as_double((long long)k);
}

template <int NPIX>
struct IxSharedT {
  uint32_t pos[NPIX];  // compacted pixels: bbox-local index | edge bit
  uint32_t key[NPIX];  // the channel's values as keys, same order
  uint32_t hist[kIxTargets][256];
  unsigned long long pref[kIxTargets];  // a target's key bits found so far
  int rank[kIxTargets];                 // its rank among the elements sharing that prefix
  int rep[kIxTargets];                  // first target with the same prefix (owns the histogram)
  int cnt[2][kIxWaves];
  double red[kIxWaves][4];
  long long redi[kIxWaves][4];
  unsigned long long redu[kIxWaves];
  uint32_t redk[kIxWaves][2];
  double med;
  // the object's geometry, read back where a channel needs it (kept out of the registers that
  // live across the channel loop)
  int n, ne;
  double ybar, xbar;
};
// the LDS-path kernel holds an object's pixels; the bbox-path kernel only the small state
template <bool LDS>
using IxShared = IxSharedT<LDS ? kIxLds : 1>;

// The object under the workgroup: plane, cut bbox and the thread's first bbox pixel and step.
struct IxObj {
  const int* lab;
  int L, H, W, r0, c0, bw, nb, n;
  int rr0, cc0, dr, dc;
};

// p in P is an edge pixel: on the plane's border, or an 8-neighbour of another label
__device__ __forceinline__ bool ix_edge(const IxObj& o, int r, int c) {
  if (r == 0 || c == 0 || r == o.H - 1 || c == o.W - 1) return true;
  const int* q = o.lab + (long long)r * o.W + c;
  const int W = o.W, L = o.L;
  return q[-W - 1] != L || q[-W] != L || q[-W + 1] != L || q[-1] != L || q[1] != L || q[W - 1] != L ||
         q[W] != L || q[W + 1] != L;
}

// f(p, rr, cc, edge) for the object's pixels of the bbox sweep p = tid, tid + 384, ...
template <bool EDGE, class F>
__device__ __forceinline__ void ix_sweep(const IxObj& o, F f) {
  int rr = o.rr0, cc = o.cc0;
  for (int p = threadIdx.x; p < o.nb; p += kIxThreads) {
    const int r = o.r0 + rr, c = o.c0 + cc;
    if (o.lab[(long long)r * o.W + c] == o.L) f(p, rr, cc, EDGE ? ix_edge(o, r, c) : false);
    rr += o.dr;
    cc += o.dc;
    if (cc >= o.bw) {
      cc -= o.bw;
      rr += 1;
    }
  }
}

// f(key, edge) for every pixel of the object: from LDS, or from the bbox
template <bool LDS, bool EDGE, class F>
__device__ __forceinline__ void ix_each_key(const IxShared<LDS>& s, const IxObj& o, const float* img, F f) {
  if (LDS) {
    for (int i = threadIdx.x; i < o.n; i += kIxThreads) f(s.key[i], EDGE ? (s.pos[i] & kEdgeBit) != 0 : false);
  } else {
    ix_sweep<EDGE>(o, [&](int, int rr, int cc, bool e) {
      f(ix_key(img[(long long)(o.r0 + rr) * o.W + (o.c0 + cc)]), e);
    });
  }
}

// Sum of v over the workgroup in wave order, in every thread (two barriers; s.red[.][slot]).
template <class S>
__device__ __forceinline__ void ix_block_sum4(S& s, double (&v)[4]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = wave_sum(v[j]);
    if (lane == 0) s.red[wave][j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double r = s.red[0][j];
#pragma unroll
    for (int w = 1; w < kIxWaves; ++w) r += s.red[w][j];
    v[j] = r;
  }
  __syncthreads();
}

// Radix select, most significant byte first: on entry s.rank[t] is target t's rank among all n
// elements, s.pref[t] = 0 and s.rep[t] = 0; on return s.pref[t] is the key of that rank.
// K is the key type (NPASS bytes), map turns an element's u32 value key into it.
template <bool LDS, int NT, int NPASS, typename K, class Map>
__device__ __forceinline__ void ix_select(IxShared<LDS>& s, const IxObj& o, const float* img, Map map) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll 1
  for (int d = 0; d < NPASS; ++d) {
    const int shift = 8 * (NPASS - 1 - d);
    for (int j = threadIdx.x; j < NT * 256; j += kIxThreads) (&s.hist[0][0])[j] = 0u;
    K hi[NT];      // the bits above this pass's byte
    bool own[NT];  // the target owns a histogram
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      hi[t] = d == 0 ? (K)0 : (K)(s.pref[t] >> (shift + 8));
      own[t] = s.rep[t] == t;
    }
    __syncthreads();
    ix_each_key<LDS, false>(s, o, img, [&](uint32_t k32, bool) {
      const K k = map(k32);
      const K khi = d == 0 ? (K)0 : (K)(k >> (shift + 8));
      const int digit = (int)((k >> shift) & 255);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (own[t] && khi == hi[t]) atomicAdd(&s.hist[t][digit], 1u);
    });
    __syncthreads();
    // one wave per target: the byte whose cumulative count passes the rank
    for (int t = wave; t < NT; t += kIxWaves) {
      const uint32_t* h = s.hist[s.rep[t]];
      const int rank = s.rank[t];
      const int c0 = (int)h[4 * lane], c1 = (int)h[4 * lane + 1], c2 = (int)h[4 * lane + 2],
                c3 = (int)h[4 * lane + 3];
      const int mine = c0 + c1 + c2 + c3;
      int incl = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
      }
      const int excl = incl - mine;
      if (excl <= rank && rank < incl) {
        int below = excl, digit = 4 * lane;
        if (rank >= below + c0) {
          below += c0;
          digit += 1;
          if (rank >= below + c1) {
            below += c1;
            digit += 1;
            if (rank >= below + c2) {
              below += c2;
              digit += 1;
            }
          }
        }
        s.pref[t] |= (unsigned long long)digit << shift;
        s.rank[t] = rank - below;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < NT) {
      int r = threadIdx.x;
      for (int j = (int)threadIdx.x - 1; j >= 0; --j)
        if (s.pref[j] == s.pref[threadIdx.x]) r = j;
      s.rep[threadIdx.x] = r;
    }
    __syncthreads();
  }
}

// CellProfiler's quantile of a sorted sequence from its two picked neighbours: t = n * f = num / 4
__device__ __forceinline__ double ix_quantile(double vi, double vi1, int num, int n) {
  const int i = num >> 2;
  const double g = (double)(num & 3) * 0.25;
  return i < n - 1 ? vi * (1.0 - g) + vi1 * g : vi;
}

template <bool LDS>
__device__ __forceinline__ void ix_channel(IxShared<LDS>& s, const IxObj& o, const float* img, double* q) {
  // ---- sums, maximum and its place, edge minimum and maximum ---------------------------------
  double sum[4] = {0.0, 0.0, 0.0, 0.0};  // x, r x, c x, x over E
  unsigned long long top = 0ull;         // key << 32 | (2^31 - 1 - p): largest key, first place
  uint32_t kmin = kNanKey, kmax = 0u;
  auto add = [&](int p, int rr, int cc, bool e, float xf) {
    const double x = (double)xf;
    const uint32_t k = ix_key(xf);
    sum[0] += x;
    sum[1] += (double)(o.r0 + rr) * x;
    sum[2] += (double)(o.c0 + cc) * x;
    const unsigned long long t = (unsigned long long)k << 32 | (uint32_t)(0x7FFFFFFF - p);
    top = t > top ? t : top;
    if (e) {
      sum[3] += x;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
    return k;
  };
  if (LDS) {
    for (int i = threadIdx.x; i < o.n; i += kIxThreads) {
      const uint32_t w = s.pos[i];
      const int p = (int)(w & ~kEdgeBit);
      const int rr = p / o.bw, cc = p - rr * o.bw;
      s.key[i] = add(p, rr, cc, (w & kEdgeBit) != 0, img[(long long)(o.r0 + rr) * o.W + (o.c0 + cc)]);
    }
  } else {
    ix_sweep<true>(o, [&](int p, int rr, int cc, bool e) {
      add(p, rr, cc, e, img[(long long)(o.r0 + rr) * o.W + (o.c0 + cc)]);
    });
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  top = wave_max(top);
  kmin = wave_min(kmin);
  kmax = wave_max(kmax);
  if (lane == 0) {
    s.redu[wave] = top;
    s.redk[wave][0] = kmin;
    s.redk[wave][1] = kmax;
  }
  ix_block_sum4(s, sum);  // (its barriers also publish redu / redk and the keys in LDS)
#pragma unroll
  for (int w = 0; w < kIxWaves; ++w) {
    top = s.redu[w] > top ? s.redu[w] : top;
    kmin = s.redk[w][0] < kmin ? s.redk[w][0] : kmin;
    kmax = s.redk[w][1] > kmax ? s.redk[w][1] : kmax;
  }
  // ---- edge variance (two-pass) ---------------------------------------------------------------
  const double mean_e = sum[3] / (double)s.ne;
  double var[4] = {0.0, 0.0, 0.0, 0.0};
  ix_each_key<LDS, true>(s, o, img, [&](uint32_t k, bool e) {
    if (e) {
      const double d = (double)ix_val(k) - mean_e;
      var[0] += d * d;
    }
  });
  ix_block_sum4(s, var);
  if (threadIdx.x == 0) {
    const int pmax = 0x7FFFFFFF - (int)(uint32_t)top;
    const int rmax = pmax / o.bw;
    const double cmy = sum[1] / sum[0], cmx = sum[2] / sum[0];
    const double dy = s.ybar - cmy, dx = s.xbar - cmx;
    q[CPX_IEXT_INTEGRATED_EDGE] = sum[3];
    q[CPX_IEXT_MEAN_EDGE] = mean_e;
    q[CPX_IEXT_STD_EDGE] = sqrt(var[0] / (double)s.ne);
    // numpy.min / numpy.max: a NaN in E (the largest key) is the result of both
    q[CPX_IEXT_MIN_EDGE] = (double)ix_val(kmax == kNanKey ? kNanKey : kmin);
    q[CPX_IEXT_MAX_EDGE] = (double)ix_val(kmax);
    q[CPX_IEXT_MASS_DISPLACEMENT] = sqrt(dy * dy + dx * dx);
    q[CPX_IEXT_CENTER_MASS_X] = cmx;
    q[CPX_IEXT_CENTER_MASS_Y] = cmy;
    q[CPX_IEXT_MAX_X] = (double)(o.c0 + pmax - rmax * o.bw);
    q[CPX_IEXT_MAX_Y] = (double)(o.r0 + rmax);
  }
  // ---- quartiles and median: ranks floor(n f) and their successors ----------------------------
  if ((int)threadIdx.x < kIxTargets) {
    const int n = s.n;
    const int num = (1 + ((int)threadIdx.x >> 1)) * n;  // 4 n f
    s.rank[threadIdx.x] = min((num >> 2) + ((int)threadIdx.x & 1), n - 1);
    s.pref[threadIdx.x] = 0ull;
    s.rep[threadIdx.x] = 0;
  }
  __syncthreads();
  ix_select<LDS, kIxTargets, 4, uint32_t>(s, o, img, [](uint32_t k) { return k; });
  if (threadIdx.x == 0) {
    const int n = s.n;
    double v[kIxTargets];
#pragma unroll
    for (int t = 0; t < kIxTargets; ++t) v[t] = (double)ix_val((uint32_t)s.pref[t]);
    q[CPX_IEXT_LOWER_QUARTILE] = ix_quantile(v[0], v[1], n, n);
    const double med = ix_quantile(v[2], v[3], 2 * n, n);
    q[CPX_IEXT_MEDIAN] = med;
    q[CPX_IEXT_UPPER_QUARTILE] = ix_quantile(v[4], v[5], 3 * n, n);
    s.med = med;
  }
  __syncthreads();
  // ---- MAD: the same quantile of |x - median| -------------------------------------------------
  const double med = s.med;
  if ((int)threadIdx.x < 2) {  // (thread 0 read the picked keys before the barrier above)
    const int n = s.n;
    s.rank[threadIdx.x] = min((n >> 1) + (int)threadIdx.x, n - 1);
    s.pref[threadIdx.x] = 0ull;
    s.rep[threadIdx.x] = 0;
  }
  __syncthreads();
  ix_select<LDS, 2, 8, unsigned long long>(
      s, o, img, [med](uint32_t k) { return ix_dkey(fabs((double)ix_val(k) - med)); });
  if (threadIdx.x == 0) q[CPX_IEXT_MAD] = ix_quantile(ix_dval(s.pref[0]), ix_dval(s.pref[1]), 2 * s.n, s.n);
  __syncthreads();  // (the next channel rewrites key, pref and rank)
}

// LDS = true measures the objects of up to CPX_IEXT_LDS_PIXELS pixels, LDS = false the others;
// each kernel passes over the objects of the other one after counting them.
template <bool LDS>
__global__ __launch_bounds__(kIxThreads, 3) void k_intensity_ext(const int* __restrict__ labels,
                                                                 const float* __restrict__ corr, int C, int H, int W,
                                                                 int max_label,
                                                                 const cpx_object* __restrict__ objects,
                                                                 const cpx_fov_objects* __restrict__ hdr,
                                                                 double* __restrict__ out) {
  __shared__ IxShared<LDS> s;
  const int fov = blockIdx.y;
  const int n_obj = min(hdr[fov].n_objects, max_label);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long N = (long long)H * W;
  for (int k = blockIdx.x; k < n_obj; k += gridDim.x) {
    const cpx_object ob = objects[(long long)fov * max_label + k];
    IxObj o;
    o.lab = labels + (long long)fov * N;
    o.L = ob.label;
    o.H = H;
    o.W = W;
    // (a table row is trusted for its label, never for addresses: the bbox is cut to the plane)
    o.r0 = max(ob.bbox[0], 0);
    o.c0 = max(ob.bbox[1], 0);
    o.bw = max(min(ob.bbox[3], W) - o.c0, 0);
    const int bh = max(min(ob.bbox[2], H) - o.r0, 0);
    o.nb = bh * o.bw;  // <= H * W < 2^31
    if (!LDS && o.nb <= kIxLds) continue;  // (before any barrier or LDS write of this object)
    o.dr = o.bw ? kIxThreads / o.bw : 0;
    o.dc = o.bw ? kIxThreads % o.bw : 0;
    o.rr0 = o.bw ? (int)threadIdx.x / o.bw : 0;
    o.cc0 = o.bw ? (int)threadIdx.x % o.bw : 0;
    // ---- geometry: n, |E|, sum r, sum c; the LDS path's compaction -----------------------------
    long long geo[4] = {0, 0, 0, 0};  // |E|, sum r, sum c, n (bbox path)
    int n = 0;
    if (LDS) {
      int rr = o.rr0, cc = o.cc0, buf = 0;
      // (uniform trip count and exit: barriers inside)
      for (int base = 0; base < o.nb && n <= kIxLds; base += kIxThreads) {
        const int p = base + (int)threadIdx.x;
        bool in = false, e = false;
        if (p < o.nb) {
          const int r = o.r0 + rr, c = o.c0 + cc;
          in = o.lab[(long long)r * W + c] == o.L;
          if (in) {
            e = ix_edge(o, r, c);
            geo[0] += e;
            geo[1] += r;
            geo[2] += c;
          }
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) s.cnt[buf][wave] = __popcll(m);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kIxWaves; ++w) {
          const int c = s.cnt[buf][w];
          before += w < wave ? c : 0;
          tot += c;
        }
        if (in) {
          const int i = n + before + __popcll(m & ((1ull << lane) - 1ull));
          if (i < kIxLds) s.pos[i] = (uint32_t)p | (e ? kEdgeBit : 0u);
        }
        n += tot;
        buf ^= 1;  // (the next chunk's counts go to the other buffer: one barrier per chunk)
        rr += o.dr;
        cc += o.dc;
        if (cc >= o.bw) {
          cc -= o.bw;
          rr += 1;
        }
      }
    } else {
      ix_sweep<true>(o, [&](int, int rr, int cc, bool e) {
        geo[0] += e;
        geo[1] += o.r0 + rr;
        geo[2] += o.c0 + cc;
        geo[3] += 1;
      });
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      geo[j] = wave_sum(geo[j]);
      if (lane == 0) s.redi[wave][j] = geo[j];
    }
    __syncthreads();  // (also publishes pos)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long long r = 0;
#pragma unroll
      for (int w = 0; w < kIxWaves; ++w) r += s.redi[w][j];
      geo[j] = r;
    }
    __syncthreads();  // (cnt and redi are free for the next object, whichever way this one goes)
    if (!LDS) n = (int)geo[3];
    if (LDS ? n > kIxLds : n <= kIxLds) continue;  // the other kernel's object
    o.n = n;
    double* row = out + ((long long)fov * max_label + k) * ((long long)CPX_N_IEXT * C);
    if (n <= 0) {
      // a table row whose label is not in its (cut) bbox: no pixel, every column NaN
      if (threadIdx.x == 0)
        for (int j = 0; j < CPX_N_IEXT * C; ++j) row[j] = (double)__uint_as_float(0x7FC00000u);
      continue;
    }
    if (threadIdx.x == 0) {
      s.n = n;
      s.ne = (int)geo[0];
      s.ybar = (double)geo[1] / (double)n;
      s.xbar = (double)geo[2] / (double)n;
    }
    __syncthreads();
    for (int c = 0; c < C; ++c) ix_channel<LDS>(s, o, corr + ((long long)fov * C + c) * N, row + CPX_N_IEXT * c);
  }
}

}  // namespace

extern "C" int cpx_n_intensity_ext(int C) { return C > 0 ? CPX_N_IEXT * C : 0; }

extern "C" int cpx_intensity_ext(cpx_ctx* ctx, const int32_t* labels_dev, const float* corr_dev, int B, int C,
                                 int H, int W, int max_label, const cpx_object* objects_dev,
                                 const cpx_fov_objects* hdr_dev, double* out_dev) {
  CPX_REQUIRE(ctx, CPX_ERR_ARG, "cpx_intensity_ext: null context");
  CPX_REQUIRE(C >= 1, CPX_ERR_ARG, "cpx_intensity_ext: %d channels (at least 1)", C);
  CPX_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && max_label > 0 && (long long)H * W < (1ll << 31),
              CPX_ERR_ARG, "cpx_intensity_ext: bad sizes");
  CPX_REQUIRE(labels_dev && corr_dev && objects_dev && hdr_dev && out_dev, CPX_ERR_ARG,
              "cpx_intensity_ext: null argument");
  // workgroups of a FOV stride over its objects; two are resident per CU (LDS), four per CU over
  // the batch even out the objects' sizes
  const int per_fov = std::max(1, std::min(max_label, (4 * ctx->n_cu + B - 1) / B));
  hipLaunchKernelGGL(k_intensity_ext<true>, dim3(per_fov, B), dim3(kIxThreads), 0, ctx->stream,
                     (const int*)labels_dev, corr_dev, C, H, W, max_label, objects_dev, hdr_dev, out_dev);
  CPX_CHECK_LAUNCH("k_intensity_ext<lds>");
  hipLaunchKernelGGL(k_intensity_ext<false>, dim3(per_fov, B), dim3(kIxThreads), 0, ctx->stream,
                     (const int*)labels_dev, corr_dev, C, H, W, max_label, objects_dev, hdr_dev, out_dev);
  CPX_CHECK_LAUNCH("k_intensity_ext<bbox>");
  return CPX_OK;
}
