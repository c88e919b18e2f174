// HD95 region metric (metrics.py:311-406, getHausdorff's channel map, the distance definition getHausdorff and
// getHausdorff_KD share) for ONE sample and the three sigmoid regions WT / TC / EC at once: six binary fields
// f = 2 * region + side (side 0 = prediction `input > 0.5`, side 1 = target `!= 0`).
//
//   hd95_zero     clears the surface counters and the histograms / list counters of the workspace
//   hd95_binarise m[v] = the six mask bits of voxel v (one byte per voxel)
//   hd95_surface  per (d, h) row, one wave: the three integer Sobel responses of every field (get_sobel_kernel, zero
//                 padding 1) -> surface bits by ballot (64-bit words per 64 voxels, kept in LDS), surface counts, the
//                 byte volume of surface bits, and the exact 1D squared distance along W to the nearest surface voxel of
//                 the row (two bit scans, no envelope needed for a binary seed)
//   hd95_lines    the lower-envelope pass (Felzenszwalb-Huttenlocher, integer breakpoints) along H, then along D; one
//                 lane per line, adjacent lanes adjacent along W (coalesced); the envelope stack lives in the workspace
//                 at [entry][lane] (lane-interleaved like scratch).  The D pass writes nothing back: at the voxels of the
//                 partner field's surface (the query set) it adds the final value to a histogram (unit spacing: exact
//                 int32 squared distances) or appends it to a list (anisotropic spacing: fp64)
//   hd95_coarse   (unit spacing) sums of 256 histogram bins, so that the finalise scan reads ~nbins / 256 words
//   hd95_finalise one workgroup per region: ranks floor(g), floor(g) + 1 of g = 0.95 (n - 1) from the histogram (coarse,
//                 then fine scan) or the list (radix select over the fp64 bit patterns), sqrt, numpy's _lerp, max of the two
//                 directions, 0 when either surface is empty
#include "common.h"

#include <algorithm>

#define XH_U8 3                       // uint8 / bool target storage (0 / 1 per byte)

namespace {

constexpr int HD_MAXW = 512;          // W <= 512: a row's surface bits are at most 8 words of 64
constexpr int HD_MAXL = 65535;        // H, D: envelope indices / breakpoints are packed as two 16-bit halves
constexpr long long HD_LANES_MAX = 131072;
constexpr int HD_BLOCK = 256;
constexpr int HD_PF = 8;             // line values loaded ahead per lane in the envelope passes

__device__ __forceinline__ bool tgt_nz(const float* p, long long i) { return p[i] != 0.f; }
template <int F> __device__ __forceinline__ bool tgt_nz(const h16<F>* p, long long i) { return cvt_in<F>(p[i].v) != 0.f; }
__device__ __forceinline__ bool tgt_nz(const unsigned char* p, long long i) { return p[i] != 0; }

template <typename T> __device__ __forceinline__ T hd_inf();
template <> __device__ __forceinline__ int hd_inf<int>() { return 0x7fffffff; }
template <> __device__ __forceinline__ double hd_inf<double>() { return __builtin_huge_val(); }

// first integer x at which parabola q (site q, value gq) is <= parabola p (p < q), clamped to [-1, n]
__device__ __forceinline__ int sep(int p, int gp, int q, int gq, int, int n) {
  const long long num = ((long long)gq + (long long)q * q) - ((long long)gp + (long long)p * p);
  const long long den = 2LL * (q - p);
  long long s = num >= 0 ? (num + den - 1) / den : -((-num) / den);
  return (int)(s < -1 ? -1 : s > n ? n : s);
}
// fp64 form (anisotropic spacing): the breakpoint is ceil() of a rounded quotient, so near a tie it can come out one above the
// exact value, which can keep a parabola or (via the s >= n skip) drop one that ties to rounding.  The squared distances this
// path returns are therefore exact only up to fp64 rounding, not bit-exact like the int32 path.
__device__ __forceinline__ int sep(int p, double gp, int q, double gq, double w, int n) {
  const double s = ceil(((gq + w * ((double)q * q)) - (gp + w * ((double)p * p))) / (2.0 * w * (q - p)));
  return s < -1.0 ? -1 : s > (double)n ? n : (int)s;
}

__device__ __forceinline__ int sq_w(int d, int) { return d * d; }
__device__ __forceinline__ double sq_w(int d, double w) { return w * ((double)d * d); }

// ------------------------------------------------------------------------------------------------ zero
__global__ __launch_bounds__(HD_BLOCK) void hd95_zero(unsigned* p, long long n) {
  for (long long i = (long long)blockIdx.x * HD_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * HD_BLOCK) p[i] = 0u;
}

// ------------------------------------------------------------------------------------------------ binarise
template <typename TI, typename TT>
__global__ __launch_bounds__(HD_BLOCK) void hd95_binarise(const TI* in, long long in_cs, const TT* tg, long long tg_cs,
                                                          unsigned char* m, long long N) {
  for (long long v = (long long)blockIdx.x * HD_BLOCK + threadIdx.x; v < N; v += (long long)gridDim.x * HD_BLOCK) {
    unsigned b = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      b |= (unsigned)(ldf(in, r * in_cs + v) > 0.5f) << (2 * r);
      b |= (unsigned)tgt_nz(tg, r * tg_cs + v) << (2 * r + 1);
    }
    m[v] = (unsigned char)b;
  }
}

// ------------------------------------------------------------------------------------------------ surface + W pass
// Sobel (metrics.py:273-290) as cross-correlation over the 3x3x3 neighbourhood n[a][b][c] (a along D, b along H, c along W):
//   x: sum_{a,b} s_a s_b (n[a][b][2] - n[a][b][0]),  y: sum_{a,c} s_c (n[a][2][c] - n[a][0][c]),  z: sum_{b,c} (n[2][b][c] - n[0][b][c])
// with s = (1, 2, 1).  Surface = any response non-zero.
__device__ __forceinline__ unsigned surface6(const unsigned char* m, int D, int H, int W, int d, int h, int w) {
  int gx[6] = {0, 0, 0, 0, 0, 0}, gy[6] = {0, 0, 0, 0, 0, 0}, gz[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int dd = d + a - 1;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int hh = h + b - 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int ww = w + c - 1;
        const bool in = dd >= 0 && dd < D && hh >= 0 && hh < H && ww >= 0 && ww < W;
        const unsigned v = in ? m[((long long)dd * H + hh) * W + ww] : 0u;
        const int sx = (a == 1 ? 2 : 1) * (b == 1 ? 2 : 1) * (c - 1);
        const int sy = (c == 1 ? 2 : 1) * (b - 1);
        const int sz = a - 1;
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          const int bit = (v >> f) & 1;
          gx[f] += sx * bit;
          gy[f] += sy * bit;
          gz[f] += sz * bit;
        }
      }
    }
  }
  unsigned s = 0;
#pragma unroll
  for (int f = 0; f < 6; ++f) s |= (unsigned)((gx[f] | gy[f] | gz[f]) != 0) << f;
  return s;
}

template <typename T>
__global__ __launch_bounds__(HD_BLOCK) void hd95_surface(const unsigned char* m, unsigned char* surf, T* fld, int D, int H, int W,
                                                         T wgt, unsigned long long* cnt) {
  __shared__ unsigned long long s_words[HD_BLOCK / 64][6][HD_MAXW / 64];
  __shared__ unsigned long long s_cnt[6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long N = (long long)D * H * W;
  const long long rows = (long long)D * H;             // 64-bit: D * H may pass 2^31 (both up to 65535)
  const int nch = (W + 63) >> 6;
  if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long c6[6] = {0, 0, 0, 0, 0, 0};
  for (long long row0 = (long long)blockIdx.x * (HD_BLOCK / 64); row0 < rows; row0 += (long long)gridDim.x * (HD_BLOCK / 64)) {   // uniform trip count
    const long long row = row0 + wave;
    const bool ok = row < rows;
    const int d = ok ? (int)(row / H) : 0, h = ok ? (int)(row % H) : 0;
    const long long rbase = row * W;
    for (int c = 0; c < nch; ++c) {
      const int w = c * 64 + lane;
      unsigned bits = 0;
      if (ok && w < W) {
        bits = surface6(m, D, H, W, d, h, w);
        surf[rbase + w] = (unsigned char)bits;
      }
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        const unsigned long long word = __ballot((bits >> f) & 1);
        if (lane == 0) s_words[wave][f][c] = word;
        c6[f] += __popcll(word);
      }
    }
    __syncthreads();
    if (ok) {
      for (int c = 0; c < nch; ++c) {
        const int w = c * 64 + lane;
        if (w >= W) continue;
        const int j = w >> 6, b = w & 63;
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          const unsigned long long* wd = s_words[wave][f];
          int best = 0x7fffffff;
          unsigned long long lm = wd[j] & (b == 63 ? ~0ull : ((2ull << b) - 1ull));
          for (int jj = j; ; ) {                           // nearest surface voxel at or left of w
            if (lm) { best = w - (jj * 64 + 63 - __builtin_clzll(lm)); break; }
            if (--jj < 0) break;
            lm = wd[jj];
          }
          unsigned long long rm = wd[j] & (~0ull << b);
          for (int jj = j; ; ) {                           // ... at or right of w
            if (rm) { const int r = jj * 64 + __builtin_ctzll(rm) - w; best = r < best ? r : best; break; }
            if (++jj >= nch) break;
            rm = wd[jj];
          }
          fld[f * N + rbase + w] = best == 0x7fffffff ? hd_inf<T>() : (T)sq_w(best, wgt);
        }
      }
    }
    __syncthreads();
  }
  if (lane == 0)
    for (int f = 0; f < 6; ++f) atomicAdd(&s_cnt[f], c6[f]);
  __syncthreads();
  if (threadIdx.x < 6) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ H / D passes
// Line L -> field f, outer index o in [0, O), column w in [0, Wd); voxel x of the line at f*N + o*ostride + w + x*lstride.
// Envelope entries 0..k-1 in the workspace (stk[e * NT + lane] = site | breakpoint << 16, stg[e * NT + lane] = value),
// entry k (the top) in registers.  Sites with an infinite value take no part; a site whose breakpoint against the top is
// >= n is never minimal inside the line and is skipped.
template <typename T, bool FINAL, bool UNIT>
__global__ __launch_bounds__(HD_BLOCK) void hd95_lines(T* fld, long long N, int O, long long ostride, int Wd, long long lstride, int n,
                                                       T wgt, unsigned* stk, T* stg, long long NT, const unsigned char* surf,
                                                       unsigned* hist, long long nbins, unsigned long long* lcnt, double* list) {
  const long long lane = (long long)blockIdx.x * HD_BLOCK + threadIdx.x;
  const long long total = 6LL * O * Wd;
  const T INF = hd_inf<T>();
  for (long long L = lane; L < total; L += NT) {
    const int w = (int)(L % Wd);
    const long long r = L / Wd;
    const int o = (int)(r % O), f = (int)(r / O);
    const long long sbase = (long long)o * ostride + w;
    T* line = fld + f * N + sbase;
    int k = -1, tv = 0, tz = 0;
    T tg = INF;
    for (int q0 = 0; q0 < n; q0 += HD_PF) {
      T gb[HD_PF];                                        // the next HD_PF values in flight together
#pragma unroll
      for (int u = 0; u < HD_PF; ++u) gb[u] = q0 + u < n ? line[(q0 + u) * lstride] : INF;
#pragma unroll
      for (int u = 0; u < HD_PF; ++u) {
      const int q = q0 + u;
      const T g = gb[u];
      if (!(g < INF)) continue;
      int s = 0;
      while (k >= 0) {
        s = sep(tv, tg, q, g, wgt, n);
        if (s > tz) break;
        if (--k >= 0) {                                   // pop: the entry below becomes the top
          const unsigned e = stk[k * NT + lane];
          tv = (int)(e & 0xffffu); tz = (int)(e >> 16); tg = stg[k * NT + lane];
        }
      }
      if (k < 0) s = 0;
      else if (s >= n) continue;
      if (k >= 0) { stk[k * NT + lane] = (unsigned)tv | ((unsigned)tz << 16); stg[k * NT + lane] = tg; }
      ++k; tv = q; tz = s; tg = g;
      }
    }
    if (k < 0) continue;                                  // no site: the line stays +inf (its field has no surface)
    int j = 0, cv, nz;
    T cg;
    if (k == 0) { cv = tv; cg = tg; nz = n; }
    else {
      const unsigned e = stk[lane]; cv = (int)(e & 0xffffu); cg = stg[lane];
      nz = k == 1 ? tz : (int)(stk[NT + lane] >> 16);
    }
    for (int x0 = 0; x0 < n; x0 += HD_PF) {
      unsigned char qb[HD_PF];                            // D pass: the partner's surface bits of the next HD_PF voxels
      if (FINAL) {
#pragma unroll
        for (int u = 0; u < HD_PF; ++u) qb[u] = x0 + u < n ? surf[sbase + (x0 + u) * lstride] : 0;
      }
#pragma unroll
      for (int u = 0; u < HD_PF; ++u) {
      const int x = x0 + u;
      if (x >= n) break;
      while (x >= nz) {
        ++j;
        if (j == k) { cv = tv; cg = tg; nz = n; }
        else {
          const unsigned e = stk[j * NT + lane]; cv = (int)(e & 0xffffu); cg = stg[j * NT + lane];
          nz = j + 1 == k ? tz : (int)(stk[(j + 1) * NT + lane] >> 16);
        }
      }
      const T val = (T)(sq_w(x - cv, wgt) + cg);
      if (!FINAL) {
        line[x * lstride] = val;
      } else if ((qb[u] >> (f ^ 1)) & 1) {               // a surface voxel of the partner field: a query
        if constexpr (UNIT) {
          if ((long long)val < nbins) atomicAdd(&hist[f * nbins + (long long)val], 1u);
        } else {
          const unsigned long long slot = atomicAdd(&lcnt[f], 1ull);
          list[f * N + (long long)slot] = (double)val;
        }
      }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ finalise
// coarse[f][cb] = sum of the fine bins cb * 256 .. cb * 256 + 255 of field f: one wave per coarse bin (coalesced, no atomics)
__global__ __launch_bounds__(HD_BLOCK) void hd95_coarse(const unsigned* hist, long long nb, unsigned* coarse) {
  const long long nbc = (nb + 255) >> 8;
  const long long wv = (long long)blockIdx.x * (HD_BLOCK / 64) + (threadIdx.x >> 6);
  if (wv >= 6 * nbc) return;
  const long long f = wv / nbc, cb = wv % nbc;
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long b = cb * 256 + i * 64 + (threadIdx.x & 63);
    if (b < nb) v += hist[f * nb + b];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) coarse[wv] = v;
}

// exclusive prefix sum over the workgroup (Hillis-Steele in LDS); returns this thread's exclusive sum, *total the sum of all
__device__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* s, unsigned long long* total) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < HD_BLOCK; off <<= 1) {
    const unsigned long long a = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += a;
    __syncthreads();
  }
  const unsigned long long incl = s[threadIdx.x];
  *total = s[HD_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

// value of rank k (0-based) of the squared distances in hist[0..nb) (fine bins) with coarse[0..ceil(nb / 256)) (sums of 256
// fine bins): the coarse bin holding rank k by a chunked scan, then the fine bin inside it by one scan of its 256 bins
__device__ double hist_rank(const unsigned* hist, const unsigned* coarse, long long nb, unsigned long long k, unsigned long long* s_tot,
                            double* s_res, long long* s_sel) {
  const long long nbc = (nb + 255) >> 8;
  const long long chunk = (nbc + HD_BLOCK - 1) / HD_BLOCK;
  const long long b0 = threadIdx.x * chunk, b1 = min(nbc, b0 + chunk);
  unsigned long long t = 0, tot;
  for (long long b = b0; b < b1; ++b) t += coarse[b];
  const unsigned long long lo = block_excl_scan(t, s_tot, &tot);
  if (k >= lo && k < lo + t) {
    unsigned long long acc = lo;
    for (long long b = b0; b < b1; ++b) {
      if (k < acc + coarse[b]) { s_sel[0] = b; s_sel[1] = (long long)acc; break; }
      acc += coarse[b];
    }
  }
  __syncthreads();
  const long long fb = s_sel[0] * 256 + threadIdx.x;
  const unsigned long long kk = k - (unsigned long long)s_sel[1];
  const unsigned long long v = fb < nb ? hist[fb] : 0u;
  const unsigned long long flo = block_excl_scan(v, s_tot, &tot);
  if (kk >= flo && kk < flo + v) *s_res = sqrt((double)fb);
  __syncthreads();
  const double r = *s_res;
  __syncthreads();
  return r;
}

// value of rank k of the n non-negative doubles (squared distances) in list[0..n): radix select over the bit patterns, 8 bits per round
__device__ double list_rank(const double* list, unsigned long long n, unsigned long long k, unsigned* s_h, unsigned long long* s_sel) {
  unsigned long long prefix = 0, pmask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    for (unsigned long long i = threadIdx.x; i < n; i += HD_BLOCK) {
      const unsigned long long u = (unsigned long long)__double_as_longlong(list[i]);
      if ((u & pmask) == prefix) atomicAdd(&s_h[(u >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long acc = 0;
      int dg = 0;
      for (; dg < 255; ++dg) {
        if (k < acc + s_h[dg]) break;
        acc += s_h[dg];
      }
      s_sel[0] = (unsigned long long)dg;
      s_sel[1] = acc;
    }
    __syncthreads();
    prefix |= s_sel[0] << shift;
    pmask |= 0xffull << shift;
    k -= s_sel[1];
    __syncthreads();
  }
  return __longlong_as_double((long long)prefix);
}

// np.percentile(x, 95), method 'linear': g = (n - 1) * 0.95, lerp between ranks floor(g) and floor(g) + 1 (numpy's _lerp)
template <bool UNIT>
__device__ double p95(const unsigned* hist, const unsigned* coarse, long long nb, const double* list, unsigned long long n,
                      unsigned long long* s_tot, unsigned* s_h, double* s_res, long long* s_sel) {
  const double g = (double)(n - 1) * 0.95;
  const double fl = floor(g);
  const unsigned long long i0 = (unsigned long long)fl, i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  const double t = __dsub_rn(g, fl);
  double a, b;
  if constexpr (UNIT) { a = hist_rank(hist, coarse, nb, i0, s_tot, s_res, s_sel); b = hist_rank(hist, coarse, nb, i1, s_tot, s_res, s_sel); }
  else { a = sqrt(list_rank(list, n, i0, s_h, s_tot)); b = sqrt(list_rank(list, n, i1, s_h, s_tot)); }   // squared distances
  const double diff = __dsub_rn(b, a);
  return t >= 0.5 ? __dsub_rn(b, __dmul_rn(diff, __dsub_rn(1.0, t))) : __dadd_rn(a, __dmul_rn(diff, t));
}

template <bool UNIT>
__global__ __launch_bounds__(HD_BLOCK) void hd95_finalise(const unsigned long long* cnt, const unsigned* hist, long long nb,
                                                          const unsigned long long* lcnt, const double* list, long long N,
                                                          double* out, long long* counts) {
  __shared__ unsigned long long s_tot[HD_BLOCK];
  __shared__ unsigned s_h[HD_BLOCK];
  __shared__ double s_res;
  __shared__ long long s_sel[2];
  const int r = blockIdx.x;
  const unsigned long long na = cnt[2 * r], nbb = cnt[2 * r + 1];
  if (counts && threadIdx.x < 2) counts[2 * r + threadIdx.x] = (long long)cnt[2 * r + threadIdx.x];
  if (na == 0 || nbb == 0) {                              // metrics.py:366-367: no surface points -> 0
    if (threadIdx.x == 0) out[r] = 0.0;
    return;
  }
  double res = 0.0;
  for (int side = 0; side < 2; ++side) {
    const int f = 2 * r + side;                           // distances to field f's surface, queried at the partner's surface
    const unsigned long long n = UNIT ? cnt[f ^ 1] : lcnt[f];
    const double v = p95<UNIT>(hist + (UNIT ? f * nb : 0), hist + (UNIT ? 6 * nb + f * ((nb + 255) >> 8) : 0), nb,
                                UNIT ? nullptr : list + f * N, n, s_tot, s_h, &s_res, s_sel);
    res = side == 0 ? v : (v > res ? v : res);
  }
  if (threadIdx.x == 0) out[r] = res;
}

struct HdLayout {
  long long N, NT, L, nbins, off_fld, off_surf, off_mask, off_stk, off_stg, off_cnt, off_hist, off_lcnt, off_list, bytes;
};

long long rup(long long x) { return (x + 255) & ~255LL; }

HdLayout hd_layout(int D, int H, int W, bool unit) {
  HdLayout l;
  l.N = (long long)D * H * W;
  l.L = D > H ? D : H;
  const long long lines = 6LL * (long long)W * (D > H ? D : H);
  l.NT = std::min(HD_LANES_MAX, (lines + HD_BLOCK - 1) / HD_BLOCK * HD_BLOCK);
  l.nbins = (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + 1;
  const long long tsz = unit ? 4 : 8;
  long long o = 0;
  l.off_fld = o; o += rup(6 * l.N * tsz);
  l.off_surf = o; o += rup(l.N);
  l.off_mask = o; o += rup(l.N);
  l.off_stk = o; o += rup(l.L * l.NT * 4);
  l.off_stg = o; o += rup(l.L * l.NT * tsz);
  l.off_cnt = o; o += rup(6 * 8);                       // zeroed region starts here
  l.off_hist = l.off_lcnt = l.off_list = o;
  if (unit) { l.off_hist = o; o += rup(6 * (l.nbins + ((l.nbins + 255) >> 8)) * 4); }
  else { l.off_lcnt = o; o += rup(6 * 8); l.off_list = o; o += rup(6 * l.N * 8); }
  l.bytes = o;
  return l;
}

int hd_grid(long long work, int cap) { return (int)std::max(1LL, std::min((long long)cap, (work + HD_BLOCK - 1) / HD_BLOCK)); }

template <typename T, bool UNIT>
int hd95_run(hipStream_t st, int in_dtype, const void* input, long long in_cs, int tgt_dtype, const void* target, long long tg_cs,
             int D, int H, int W, double s0, double s1, double s2, char* ws, double* out, long long* counts) {
  const HdLayout l = hd_layout(D, H, W, UNIT);
  T* fld = (T*)(ws + l.off_fld);
  unsigned char* surf = (unsigned char*)(ws + l.off_surf);
  unsigned char* m = (unsigned char*)(ws + l.off_mask);
  unsigned* stk = (unsigned*)(ws + l.off_stk);
  T* stg = (T*)(ws + l.off_stg);
  unsigned long long* cnt = (unsigned long long*)(ws + l.off_cnt);
  unsigned* hist = (unsigned*)(ws + l.off_hist);
  unsigned long long* lcnt = (unsigned long long*)(ws + l.off_lcnt);
  double* list = (double*)(ws + l.off_list);
  const long long zero_words = ((UNIT ? l.off_hist + 6 * l.nbins * 4 : l.off_lcnt + 6 * 8) - l.off_cnt) / 4;   // (coarse sums: written whole)
  hd95_zero<<<hd_grid(zero_words, 1024), HD_BLOCK, 0, st>>>((unsigned*)(ws + l.off_cnt), zero_words);
#define HD_BIN(TI)                                                                                                        \
  do {                                                                                                                    \
    if (tgt_dtype == XH_F32) hd95_binarise<TI, float><<<hd_grid(l.N, 4096), HD_BLOCK, 0, st>>>((const TI*)input, in_cs, (const float*)target, tg_cs, m, l.N); \
    else if (tgt_dtype == XH_BF16) hd95_binarise<TI, bf16_t><<<hd_grid(l.N, 4096), HD_BLOCK, 0, st>>>((const TI*)input, in_cs, (const bf16_t*)target, tg_cs, m, l.N); \
    else if (tgt_dtype == XH_F16) hd95_binarise<TI, f16_t><<<hd_grid(l.N, 4096), HD_BLOCK, 0, st>>>((const TI*)input, in_cs, (const f16_t*)target, tg_cs, m, l.N); \
    else hd95_binarise<TI, unsigned char><<<hd_grid(l.N, 4096), HD_BLOCK, 0, st>>>((const TI*)input, in_cs, (const unsigned char*)target, tg_cs, m, l.N); \
  } while (0)
  if (in_dtype == XH_F32) HD_BIN(float);
  else if (in_dtype == XH_BF16) HD_BIN(bf16_t);
  else HD_BIN(f16_t);
#undef HD_BIN
  const T w0 = (T)(s0 * s0), w1 = (T)(s1 * s1), w2 = (T)(s2 * s2);
  const long long rows = (long long)D * H;
  hd95_surface<T><<<(int)std::max(1LL, std::min(2048LL, (rows + 3) / 4)), HD_BLOCK, 0, st>>>(m, surf, fld, D, H, W, w2, cnt);
  const int gl = (int)(l.NT / HD_BLOCK);
  // H pass: lines (f, d, w), step W
  hd95_lines<T, false, UNIT><<<gl, HD_BLOCK, 0, st>>>(fld, l.N, D, (long long)H * W, W, W, H, w1, stk, stg, l.NT, surf, hist, l.nbins,
                                                      lcnt, list);
  // D pass: lines (f, h, w), step H*W; values go to the histogram / list at the query voxels
  hd95_lines<T, true, UNIT><<<gl, HD_BLOCK, 0, st>>>(fld, l.N, H, W, W, (long long)H * W, D, w0, stk, stg, l.NT, surf, hist, l.nbins,
                                                     lcnt, list);
  if (UNIT) {
    const long long nwaves = 6 * ((l.nbins + 255) >> 8);
    hd95_coarse<<<(int)((nwaves + HD_BLOCK / 64 - 1) / (HD_BLOCK / 64)), HD_BLOCK, 0, st>>>(hist, l.nbins, hist + 6 * l.nbins);
  }
  hd95_finalise<UNIT><<<3, HD_BLOCK, 0, st>>>(cnt, hist, l.nbins, lcnt, list, l.N, out, counts);
  return xh_launch_status();
}

// the exact int32 / histogram path: unit spacing and squared distances below 2^24 (BraTS: 139 k); otherwise the fp64 list path,
// which is also exact for unit spacing (integer squared distances < 2^53, correctly rounded sqrt)
bool hd_use_hist(int D, int H, int W, bool unit) {
  return unit && (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) < (1LL << 24);
}

bool hd_shape_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && W <= HD_MAXW && H <= HD_MAXL && D <= HD_MAXL; }

}  // namespace

extern "C" long long xh_hd95_workspace_bytes(int D, int H, int W, int unit_spacing) {
  if (!hd_shape_ok(D, H, W)) return -1;
  return hd_layout(D, H, W, hd_use_hist(D, H, W, unit_spacing != 0)).bytes;
}

extern "C" int xh_hd95(void* stream, int in_dtype, const void* input, long long in_cstride, int tgt_dtype, const void* target,
                       long long tgt_cstride, int D, int H, int W, double s0, double s1, double s2, void* ws, long long ws_bytes,
                       double* out, long long* counts) {
  if (!input || !target || !ws || !out || !hd_shape_ok(D, H, W)) return XH_ERR_ARG;
  if (!(s0 > 0.0) || !(s1 > 0.0) || !(s2 > 0.0)) return XH_ERR_ARG;
  const long long N = (long long)D * H * W;
  if (in_cstride < N || tgt_cstride < N) return XH_ERR_ARG;
  if (in_dtype != XH_F32 && in_dtype != XH_BF16 && in_dtype != XH_F16) return XH_ERR_DTYPE;
  if (tgt_dtype != XH_F32 && tgt_dtype != XH_BF16 && tgt_dtype != XH_F16 && tgt_dtype != XH_U8) return XH_ERR_DTYPE;
  const bool unit = hd_use_hist(D, H, W, s0 == 1.0 && s1 == 1.0 && s2 == 1.0);
  if (ws_bytes < hd_layout(D, H, W, unit).bytes) return XH_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (unit)
    return hd95_run<int, true>(st, in_dtype, input, in_cstride, tgt_dtype, target, tgt_cstride, D, H, W, 1.0, 1.0, 1.0, (char*)ws, out, counts);
  return hd95_run<double, false>(st, in_dtype, input, in_cstride, tgt_dtype, target, tgt_cstride, D, H, W, s0, s1, s2, (char*)ws, out,
                                 counts);
}
