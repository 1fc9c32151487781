// Per-object neighbour measurements (CellProfiler 4 MeasureObjectNeighbors, an object set against
// itself, "Adjacent" and "Within a specified distance"; restated in include/cpx.h and DESIGN.md
// §15): per scale D the number of other labels within the disk of radius^2 D^2 of the object, the
// percentage of its edge pixels with another label within radius^2 D^2 + D, and the two closest
// centres with the angle between them.
//
// k_nb_closest: one thread per object, the FOV's centres and labels staged through LDS in chunks of
//   256; the thread keeps the three smallest (d, j) in table order (j ascending, strict <, so the
//   lower index wins a tie: numpy's stable argsort).  O(n^2) per FOV.
// k_nb_touch: one 256-thread workgroup per object and scale.  The window (bbox grown by D, cut to
//   the plane) is walked in segments of kNbSegW columns and bands of kNbBandH rows; each tile is
//   staged with a D halo as one class byte per pixel (0 background, 1 the object, 2 another label).
//   Both tests are capped distance transforms done separably:
//     row pass    hL, hO = horizontal distance to the nearest class-1 / class-2 pixel of the row,
//                 capped at D + 1 (a byte), for the tile's core columns and all its rows
//     column pass min over |dy| <= D of dy^2 + h(y + dy)^2 at the core pixels: against D^2 with hL at
//                 a class-2 pixel (its label goes into the LDS bitmap), against D^2 + D with hO at
//                 an edge pixel of the object (counted)
//   so a window pixel costs O(D) per test.  Integer arithmetic throughout, integer LDS atomics
//   only, no workspace: two runs give the same bits.
#include "cpx_internal.h"

namespace {

constexpr int kNbThreads = 256;
constexpr int kNbWaves = kNbThreads / 64;
constexpr int kNbBandH = CPX_NEIGHBORS_BAND_ROWS;    // core rows of a tile
constexpr int kNbSegW = CPX_NEIGHBORS_SEGMENT_COLS;  // core columns of a tile
constexpr int kNbMaxD = CPX_NEIGHBORS_MAX_DISTANCE;
constexpr int kNbTileS = kNbSegW + 2 * kNbMaxD;      // class tile row stride (bytes)
constexpr int kNbTileH = kNbBandH + 2 * kNbMaxD;     // class tile rows
// dynamic LDS carve (bytes, every offset a multiple of 16)
constexpr int kNbOffCls = 0;
constexpr int kNbOffHL = kNbOffCls + kNbTileH * kNbTileS;
constexpr int kNbOffHO = kNbOffHL + kNbTileH * kNbSegW;
constexpr int kNbOffRed = kNbOffHO + kNbTileH * kNbSegW;
constexpr int kNbOffBits = kNbOffRed + 64;
static_assert(kNbOffBits % 16 == 0, "LDS carve offsets stay 16-byte aligned");
__host__ __device__ constexpr int nb_words(int max_label) { return (max_label + 32) >> 5; }
static_assert(kNbOffBits + 4 * nb_words(CPX_NEIGHBORS_MAX_LABEL) <= 65536, "the bitmap fits 64 KiB of LDS");

struct nb_scales {
  int n;
  int d[CPX_NEIGHBORS_MAX_SCALES];
};

// lanes per row for a row of `w` elements: the smallest power of two >= w within lo .. hi (log2)
__device__ __forceinline__ int nb_row_shift(int w, int lo, int hi) {
  int s = lo;
  while (s < hi && (1 << s) < w) ++s;
  return s;
}

__global__ __launch_bounds__(kNbThreads) void k_nb_touch(const int* __restrict__ labels, int H, int W,
                                                        int max_label, const cpx_object* __restrict__ objects,
                                                        const cpx_fov_objects* __restrict__ hdr, nb_scales sc,
                                                        double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_smem[];
  unsigned char* s_cls = nb_smem + kNbOffCls;  // [kNbTileH][kNbTileS]
  unsigned char* s_hl = nb_smem + kNbOffHL;    // [kNbTileH][kNbSegW]
  unsigned char* s_ho = nb_smem + kNbOffHO;
  int* s_red = (int*)(nb_smem + kNbOffRed);    // [kNbWaves][3]
  unsigned int* s_bits = (unsigned int*)(nb_smem + kNbOffBits);  // nb_words(max_label)
  const int fov = blockIdx.y;
  const int n_obj = min(hdr[fov].n_objects, max_label);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = nb_words(max_label);
  const int* lab = labels + (long long)fov * H * W;
  const int ncol = CPX_N_NEIGHBORS * sc.n;
  for (int k = blockIdx.x; k < n_obj; k += gridDim.x) {
    const cpx_object o = objects[(long long)fov * max_label + k];
    const int L = o.label;
    // (a table row is trusted for its label, never for addresses: the bbox is cut to the plane)
    const int r0 = max(o.bbox[0], 0), c0 = max(o.bbox[1], 0);
    const int r1 = min(o.bbox[2], H), c1 = min(o.bbox[3], W);
    double* q = out + ((long long)fov * max_label + k) * ncol;
    for (int s = 0; s < sc.n; ++s) {
      const int D = sc.d[s];
      const int lim_n = D * D, lim_t = D * D + D;
      const bool some = r1 > r0 && c1 > c0;
      // the window: the bbox grown by D, cut to the plane
      const int wr0 = max(r0 - D, 0), wr1 = some ? min(r1 + D, H) : wr0;
      const int wc0 = max(c0 - D, 0), wc1 = some ? min(c1 + D, W) : wc0;
      for (int i = tid; i < words; i += kNbThreads) s_bits[i] = 0u;
      int n_edge = 0, n_touch = 0;
      for (int x0 = wc0; x0 < wc1; x0 += kNbSegW) {
        const int sw = min(kNbSegW, wc1 - x0), tw = sw + 2 * D;
        for (int y0 = wr0; y0 < wr1; y0 += kNbBandH) {
          const int bh = min(kNbBandH, wr1 - y0), th = bh + 2 * D;
          __syncthreads();  // the previous tile's readers are done (and the bitmap is zeroed)
          {  // class tile with its D halo; outside the plane is background
            const int sh = nb_row_shift(tw, 5, 7);
            const int tx = tid & ((1 << sh) - 1), gx = x0 - D + tx;
            for (int ty = tid >> sh; ty < th; ty += kNbThreads >> sh) {
              const int gy = y0 - D + ty;
              if (tx < tw) {
                int l = 0;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) l = lab[(long long)gy * W + gx];
                s_cls[ty * kNbTileS + tx] = l == L ? 1 : (l >= 1 && l <= max_label) ? 2 : 0;
              }
            }
          }
          __syncthreads();
          const int sh = nb_row_shift(sw, 4, 6);
          const int cx = tid & ((1 << sh) - 1);
          if (cx < sw) {  // row pass: every tile row, core columns
            for (int ty = tid >> sh; ty < th; ty += kNbThreads >> sh) {
              const unsigned char* row = s_cls + ty * kNbTileS + cx + D;
              int hl = D + 1, ho = D + 1;
              for (int dx = 0; dx <= D; ++dx) {
                const int a = row[-dx], b = row[dx];
                if (hl > D && (a == 1 || b == 1)) hl = dx;
                if (ho > D && (a == 2 || b == 2)) ho = dx;
                if (hl <= D && ho <= D) break;
              }
              s_hl[ty * kNbSegW + cx] = (unsigned char)hl;
              s_ho[ty * kNbSegW + cx] = (unsigned char)ho;
            }
          }
          __syncthreads();
          if (cx < sw) {  // column pass: core pixels
            const int gx = x0 + cx;
            for (int cy = tid >> sh; cy < bh; cy += kNbThreads >> sh) {
              const int ty = cy + D, gy = y0 + cy;
              const unsigned char* c = s_cls + ty * kNbTileS + cx + D;
              const int cls = c[0];
              if (cls == 0) continue;
              const unsigned char* h = (cls == 2 ? s_hl : s_ho) + ty * kNbSegW + cx;
              if (cls == 1) {
                const bool edge = gy == 0 || gy == H - 1 || gx == 0 || gx == W - 1 ||
                                  c[-kNbTileS - 1] != 1 || c[-kNbTileS] != 1 || c[-kNbTileS + 1] != 1 ||
                                  c[-1] != 1 || c[1] != 1 ||
                                  c[kNbTileS - 1] != 1 || c[kNbTileS] != 1 || c[kNbTileS + 1] != 1;
                if (!edge) continue;
                n_edge += 1;
              }
              int m = h[0] * h[0];
              for (int dy = 1; dy <= D; ++dy) {
                const int u = h[-dy * kNbSegW], v = h[dy * kNbSegW];
                m = min(m, dy * dy + min(u * u, v * v));
              }
              if (cls == 2) {
                if (m <= lim_n) {
                  const int l = lab[(long long)gy * W + gx];
                  atomicOr(&s_bits[l >> 5], 1u << (l & 31));
                }
              } else if (m <= lim_t) {
                n_touch += 1;
              }
            }
          }
        }
      }
      __syncthreads();
      int n_nb = 0;
      for (int i = tid; i < words; i += kNbThreads) n_nb += __popc(s_bits[i]);
      n_nb = wave_sum(n_nb);
      n_edge = wave_sum(n_edge);
      n_touch = wave_sum(n_touch);
      if (lane == 0) {
        s_red[wave * 3 + 0] = n_nb;
        s_red[wave * 3 + 1] = n_edge;
        s_red[wave * 3 + 2] = n_touch;
      }
      __syncthreads();
      if (tid == 0) {
        long long nb = 0, ne = 0, nt = 0;
        for (int w = 0; w < kNbWaves; ++w) {
          nb += s_red[w * 3 + 0];
          ne += s_red[w * 3 + 1];
          nt += s_red[w * 3 + 2];
        }
        q[CPX_N_NEIGHBORS * s + CPX_NB_NUMBER_OF_NEIGHBORS] = (double)nb;
        q[CPX_N_NEIGHBORS * s + CPX_NB_PERCENT_TOUCHING] = ne > 0 ? (double)(nt * 100) / (double)ne : 0.0;
      }
      // (no barrier here: s_red is next written after at least one more barrier, the one that
      // follows the tile loops (an empty window has no other), and thread 0 reaches that barrier
      // only after the reads above; s_bits is zeroed for the next scale only by threads that have
      // passed the barrier above, after every popcount read)
    }
  }
}

// insert (d, j) into the ascending triple; j arrives in ascending order, so strict < keeps the
// lower index first among equal distances
__device__ __forceinline__ void nb_insert(double d, int j, double (&bd)[3], int (&bj)[3]) {
  if (d < bd[2]) {
    if (d < bd[1]) {
      bd[2] = bd[1];
      bj[2] = bj[1];
      if (d < bd[0]) {
        bd[1] = bd[0];
        bj[1] = bj[0];
        bd[0] = d;
        bj[0] = j;
      } else {
        bd[1] = d;
        bj[1] = j;
      }
    } else {
      bd[2] = d;
      bj[2] = j;
    }
  }
}

__global__ __launch_bounds__(kNbThreads) void k_nb_closest(int max_label, const cpx_object* __restrict__ objects,
                                                          const cpx_fov_objects* __restrict__ hdr, int n_scales,
                                                          double* __restrict__ out) {
  __shared__ double s_r[kNbThreads], s_c[kNbThreads];
  const int fov = blockIdx.y;
  const int n = min(hdr[fov].n_objects, max_label);
  const cpx_object* tab = objects + (long long)fov * max_label;
  const int ncol = CPX_N_NEIGHBORS * n_scales;
  for (int base = blockIdx.x * kNbThreads; base < n; base += gridDim.x * kNbThreads) {
    const int k = base + threadIdx.x;
    double kr = 0.0, kc = 0.0;
    if (k < n) {
      kr = tab[k].centroid_r;
      kc = tab[k].centroid_c;
    }
    double bd[3] = {INFINITY, INFINITY, INFINITY};
    int bj[3] = {-1, -1, -1};
    for (int j0 = 0; j0 < n; j0 += kNbThreads) {
      __syncthreads();
      if (j0 + (int)threadIdx.x < n) {
        s_r[threadIdx.x] = tab[j0 + threadIdx.x].centroid_r;
        s_c[threadIdx.x] = tab[j0 + threadIdx.x].centroid_c;
      }
      __syncthreads();
      if (k < n) {
        const int m = min(kNbThreads, n - j0);
        for (int jj = 0; jj < m; ++jj) {
          // each square and the sum rounded on their own (the unit is built with contraction off)
          const double dr = kr - s_r[jj], dc = kc - s_c[jj];
          nb_insert(__dsqrt_rn(dr * dr + dc * dc), j0 + jj, bd, bj);
        }
      }
    }
    if (k < n) {
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // first number, distance, second number, distance, angle
      if (n >= 2) {
        const cpx_object a = tab[bj[1]];
        v[0] = (double)a.label;
        v[1] = bd[1];
        if (n >= 3) {
          const cpx_object b = tab[bj[2]];
          v[2] = (double)b.label;
          v[3] = bd[2];
          const double v1r = a.centroid_r - kr, v1c = a.centroid_c - kc;
          const double v2r = b.centroid_r - kr, v2c = b.centroid_c - kc;
          v[4] = atan2(fabs(v1c * v2r - v1r * v2c), v1r * v2r + v1c * v2c) * (180.0 / 3.14159265358979323846);
        }
      }
      double* q = out + ((long long)fov * max_label + k) * ncol;
      for (int s = 0; s < n_scales; ++s)
        for (int i = 0; i < 5; ++i) q[CPX_N_NEIGHBORS * s + CPX_NB_FIRST_CLOSEST_OBJECT_NUMBER + i] = v[i];
    }
  }
}

}  // namespace

extern "C" int cpx_n_neighbors(int n_scales) { return n_scales > 0 ? CPX_N_NEIGHBORS * n_scales : 0; }

extern "C" int cpx_neighbors(cpx_ctx* ctx, const int32_t* labels_dev, int B, int H, int W, int max_label,
                             const cpx_object* objects_dev, const cpx_fov_objects* hdr_dev, const int* distances,
                             int n_scales, double* out_dev) {
  CPX_REQUIRE(ctx, CPX_ERR_ARG, "cpx_neighbors: null context");
  CPX_REQUIRE(n_scales >= 1 && n_scales <= CPX_NEIGHBORS_MAX_SCALES, CPX_ERR_ARG,
              "cpx_neighbors: %d scales (1 .. %d supported)", n_scales, CPX_NEIGHBORS_MAX_SCALES);
  CPX_REQUIRE(distances, CPX_ERR_ARG, "cpx_neighbors: null distances");
  nb_scales sc;
  sc.n = n_scales;
  for (int s = 0; s < CPX_NEIGHBORS_MAX_SCALES; ++s) {
    sc.d[s] = s < n_scales ? distances[s] : 1;
    CPX_REQUIRE(sc.d[s] >= 1 && sc.d[s] <= CPX_NEIGHBORS_MAX_DISTANCE, CPX_ERR_ARG,
                "cpx_neighbors: distance %d (1 .. %d supported)", sc.d[s], CPX_NEIGHBORS_MAX_DISTANCE);
  }
  CPX_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && max_label > 0, CPX_ERR_ARG, "cpx_neighbors: bad sizes");
  CPX_REQUIRE(max_label <= CPX_NEIGHBORS_MAX_LABEL, CPX_ERR_ARG,
              "cpx_neighbors: max_label %d (the label bitmap holds at most %d)", max_label,
              CPX_NEIGHBORS_MAX_LABEL);
  CPX_REQUIRE(labels_dev && objects_dev && hdr_dev && out_dev, CPX_ERR_ARG, "cpx_neighbors: null argument");
  // workgroups of a FOV stride over its objects; ~8 resident workgroups per CU over the batch
  const int per_fov = std::max(1, std::min(max_label, (8 * ctx->n_cu + B - 1) / B));
  const size_t lds = (size_t)kNbOffBits + sizeof(unsigned int) * nb_words(max_label);
  hipLaunchKernelGGL(k_nb_touch, dim3(per_fov, B), dim3(kNbThreads), lds, ctx->stream, (const int*)labels_dev, H, W,
                     max_label, objects_dev, hdr_dev, sc, out_dev);
  CPX_CHECK_LAUNCH("k_nb_touch");
  const int cgrid = std::min(cpx_div_up(max_label, kNbThreads), 1024);
  hipLaunchKernelGGL(k_nb_closest, dim3(cgrid, B), dim3(kNbThreads), 0, ctx->stream, max_label, objects_dev, hdr_dev,
                     n_scales, out_dev);
  CPX_CHECK_LAUNCH("k_nb_closest");
  return CPX_OK;
}
