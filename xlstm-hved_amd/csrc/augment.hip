// Training-time augmentation on device-resident volumes (transform.py:10-28 with train.py:121's configuration; the C ABI and
// the exact word -> parameter mapping are documented in include/xlstm_hved.h).
//
//   xh_aug_moments   once per registered volume: count / mean / std (ddof 0) of each channel's nonzero voxels, fp64, fixed
//                    reduction order (per-block partials, then one workgroup per channel folds them in index order)
//   xh_aug_draw      per batch: Philox4x32-10 parameter draws for N samples, one workgroup, advances the device counter
//   xh_aug_apply     per batch: one gather launch building x (N, 4, d, h, w) and the SegToMask mask (N, 3, d, h, w)
//
// apply is a streaming kernel: every output voxel reads 4 source values and one label byte and writes 4 + 3 values.  A thread
// owns 4 consecutive voxels of the flattened output (h, w) plane of one (sample, z); rows run along W, which never flips, so a
// wave's loads of one channel are consecutive addresses of <= 2 source rows and its stores are one contiguous 16-B-per-lane
// (fp32) or 8-B-per-lane (16-bit) segment.
#include "common.h"
#include "../../include/xlstm_hved.h"

// Every operation of the draws and of the voxel arithmetic rounds once, as documented in the header (and as numpy does):
// without it the compiler fuses a * b + c into one fma (the _rn intrinsics do not prevent that: they are inline operators
// compiled under the default contraction).
#pragma clang fp contract(off)

#define AUG_FLAG_SCALE XH_AUG_SCALE
#define AUG_FLAG_SHIFT XH_AUG_SHIFT
#define AUG_FLAG_FLIP XH_AUG_FLIP
#define AUG_FLAG_NORM XH_AUG_NORMALIZE

namespace {

// ------------------------------------------------------------------------------------------------ moments
constexpr int MOM_T = 256;
constexpr int MOM_MAXB = 512;          // partial blocks per channel

inline int mom_blocks(long long n) {
  long long b = (n + (long long)MOM_T * 64 - 1) / ((long long)MOM_T * 64);
  return (int)(b < 1 ? 1 : (b > MOM_MAXB ? MOM_MAXB : b));
}

__device__ __forceinline__ float src_f(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float src_f(const short* p, long long i) { return (float)p[i]; }

__device__ __forceinline__ void acc(float v, unsigned long long& c, double& s1, double& s2) {
  if (v != 0.f) {
    const double d = (double)v;
    c += 1; s1 += d; s2 = fma(d, d, s2);
  }
}

// fixed-order block reduction of (count, sum, sumsq): wave butterflies, then wave 0 folds the 4 wave results in order
__device__ __forceinline__ void block_reduce3(unsigned long long& c, double& s1, double& s2) {
  __shared__ double sh[3][MOM_T / 64];
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o);
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][wv] = (double)c; sh[1][wv] = s1; sh[2][wv] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0, b = 0, q = 0;
    for (int k = 0; k < MOM_T / 64; ++k) { a += sh[0][k]; b += sh[1][k]; q += sh[2][k]; }
    c = (unsigned long long)a; s1 = b; s2 = q;
  }
}

// partials[(c * nb + b) * 3 + {0, 1, 2}] = {count, sum, sumsq} of block b's contiguous chunk of channel c (blockIdx.y)
template <typename S, bool VEC>
__global__ __launch_bounds__(MOM_T) void aug_moments_partial_kernel(const S* __restrict__ img, long long n, long long chunk,
                                                                      double* __restrict__ part) {
  const int c = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
  const S* p = img + (long long)c * n;
  const long long lo = (long long)b * chunk, hi = lo + chunk < n ? lo + chunk : n;
  unsigned long long cnt = 0;
  double s1 = 0.0, s2 = 0.0;
  if constexpr (VEC) {
    // chunk is a multiple of 8 elements and channel bases are 16-B aligned (n % (16 / sizeof(S)) == 0): 16 B per lane
    constexpr int V = 16 / sizeof(S);
    for (long long i = lo + (long long)threadIdx.x * V; i < hi; i += (long long)MOM_T * V) {
      const uint4 u = *reinterpret_cast<const uint4*>(p + i);
      if constexpr (sizeof(S) == 4) {
        acc(__uint_as_float(u.x), cnt, s1, s2); acc(__uint_as_float(u.y), cnt, s1, s2);
        acc(__uint_as_float(u.z), cnt, s1, s2); acc(__uint_as_float(u.w), cnt, s1, s2);
      } else {
        const unsigned w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc((float)(short)(w4[k] & 0xFFFFu), cnt, s1, s2);
          acc((float)(short)(w4[k] >> 16), cnt, s1, s2);
        }
      }
    }
  } else {
    for (long long i = lo + threadIdx.x; i < hi; i += MOM_T) acc(src_f(p, i), cnt, s1, s2);
  }
  block_reduce3(cnt, s1, s2);
  if (threadIdx.x == 0) {
    double* o = part + ((long long)c * nb + b) * 3;
    o[0] = (double)cnt; o[1] = s1; o[2] = s2;
  }
}

__global__ __launch_bounds__(MOM_T) void aug_moments_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  const int c = blockIdx.x;
  unsigned long long cnt = 0;
  double s1 = 0.0, s2 = 0.0;
  for (int b = threadIdx.x; b < nb; b += MOM_T) {
    const double* q = part + ((long long)c * nb + b) * 3;
    cnt += (unsigned long long)q[0]; s1 += q[1]; s2 += q[2];
  }
  block_reduce3(cnt, s1, s2);
  if (threadIdx.x == 0) {
    double mean = 0.0, sd = 0.0;
    if (cnt > 0) {
      const double nn = (double)cnt;
      mean = s1 / nn;
      const double var = s2 / nn - mean * mean;      // fp64 sums: cancellation ~1e-16 (mean / std)^2, far below the fp32 output
      sd = var > 0.0 ? sqrt(var) : 0.0;
    }
    out[4 * c + 0] = (double)cnt; out[4 * c + 1] = mean; out[4 * c + 2] = sd; out[4 * c + 3] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ draws
__device__ __forceinline__ unsigned long long w64(unsigned a, unsigned b) { return ((unsigned long long)a << 32) | b; }
__device__ __forceinline__ double u53(unsigned a, unsigned b) { return (double)(w64(a, b) >> 11) * 0x1p-53; }
__device__ __forceinline__ int ranged(unsigned a, unsigned b, int r) { return (int)__umul64hi(w64(a, b), (unsigned long long)r); }
__device__ __forceinline__ double unif(double lo, double width, double u) { return lo + width * u; }

__global__ __launch_bounds__(256) void aug_draw_kernel(const xh_aug_volume* __restrict__ vols, int nvol, const int* __restrict__ idx,
                                                       int N, int cd, int ch, int cw, int flags, double s_scale, double s_shift,
                                                       double p, unsigned long long* rng, xh_aug_params* __restrict__ out) {
  PhiloxKey k;
  k.seed = rng[0]; k.ctr = rng[1]; k.stream = XH_AUG_RNG_STREAM;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    unsigned b0[4], b1[4], b2[4], b3[4];
    philox_block(k, 4ll * n + 0, b0);
    philox_block(k, 4ll * n + 1, b1);
    philox_block(k, 4ll * n + 2, b2);
    philox_block(k, 4ll * n + 3, b3);
    xh_aug_params q;
    q.scale = (flags & AUG_FLAG_SCALE) ? unif(1.0 - s_scale, 2.0 * s_scale, u53(b0[0], b0[1])) : 1.0;
    q.shift = (flags & AUG_FLAG_SHIFT) ? unif(-s_shift, 2.0 * s_shift, u53(b0[2], b0[3])) : 0.0;
    q.flip = (flags & AUG_FLAG_FLIP) ? ((u53(b2[2], b2[3]) > p ? 1 : 0) | (u53(b3[0], b3[1]) > p ? 2 : 0)) : 0;
    const int v = idx[n];
    if (v < 0 || v >= nvol) {
      q.origin[0] = q.origin[1] = q.origin[2] = -1;
    } else {
      const int rd = vols[v].D - cd, rh = vols[v].H - ch, rw = vols[v].W - cw;
      if (rd < 0 || rh < 0 || rw < 0) {
        q.origin[0] = q.origin[1] = q.origin[2] = -1;
      } else {
        q.origin[0] = ranged(b1[0], b1[1], rd);
        q.origin[1] = ranged(b1[2], b1[3], rh);
        q.origin[2] = ranged(b2[0], b2[1], rw);
      }
    }
    out[n] = q;
  }
  // every lane has read the counter above; the barrier orders those reads before the advance
  __syncthreads();
  if (threadIdx.x == 0) rng[1] = k.ctr + 1;
}

// ------------------------------------------------------------------------------------------------ apply
constexpr int AP_T = 256;
constexpr int AP_PER = 4;                  // consecutive output voxels per thread
constexpr int AP_TILE = AP_T * AP_PER;     // output voxels of one (n, z) plane per workgroup

__device__ __forceinline__ void st_out(float* p, long long i, float v) { p[i] = v; }
template <int F> __device__ __forceinline__ void st_out(h16<F>* p, long long i, float v) { p[i].v = cvt_out<F>(v); }

template <typename XT, typename MT>
__global__ __launch_bounds__(AP_T) void aug_apply_kernel(const xh_aug_volume* __restrict__ vols, int nvol,
                                                         const double* __restrict__ mom, const int* __restrict__ idx,
                                                         const xh_aug_params* __restrict__ prm, int d, int h, int w, int flags,
                                                         XT* __restrict__ x, MT* __restrict__ mask, bool vec) {
  const int n = blockIdx.z, z = blockIdx.y;
  const long long hw = (long long)h * w, dhw = hw * d;
  const int p0 = (blockIdx.x * AP_T + threadIdx.x) * AP_PER;
  if (p0 >= hw) return;
  const long long obase = (long long)z * hw + p0;
  XT* xo = x + (long long)n * 4 * dhw + obase;
  MT* mo = mask + (long long)n * 3 * dhw + obase;
  const int cnt = hw - p0 < AP_PER ? (int)(hw - p0) : AP_PER;
  const bool v4 = vec && cnt == AP_PER;

  const int v = idx[n];
  const xh_aug_params q = prm[n];
  bool ok = v >= 0 && v < nvol;
  xh_aug_volume vol = {nullptr, nullptr, 0, 0, 0, 0};
  if (ok) {
    vol = vols[v];
    ok = q.origin[0] >= 0 && q.origin[1] >= 0 && q.origin[2] >= 0 && q.origin[0] + d <= vol.D && q.origin[1] + h <= vol.H &&
         q.origin[2] + w <= vol.W;
  }
  float xv[4][AP_PER], mv[3][AP_PER];
  if (!ok) {                               // invalid parameters: NaN image, empty mask, no source access
#pragma unroll
    for (int k = 0; k < AP_PER; ++k) {
      xv[0][k] = xv[1][k] = xv[2][k] = xv[3][k] = __int_as_float(0x7fc00000);
      mv[0][k] = mv[1][k] = mv[2][k] = 0.f;
    }
  } else {
    const long long DHW = (long long)vol.D * vol.H * vol.W;
    const int zz = q.origin[0] + z;
    const int zs = (q.flip & 1) ? vol.D - 1 - zz : zz;
    const bool f32 = vol.dtype == XH_F32;           // per sample (workgroup-uniform): a batch may mix fp32 and int16 volumes
    const bool do_scale = flags & AUG_FLAG_SCALE, do_shift = flags & AUG_FLAG_SHIFT, do_norm = flags & AUG_FLAG_NORM;
    const float a_scale = (float)q.scale, a_shift = (float)q.shift;
    float shift_c[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)            // np.std of the scaled channel (a_scale > 0 keeps the nonzero set), times alpha, in fp32
      shift_c[c] = (float)((double)a_scale * mom[((long long)v * 4 + c) * 4 + 2]) * a_shift;
    int y = p0 / w, u = p0 - y * w;
    long long off[AP_PER];
#pragma unroll
    for (int k = 0; k < AP_PER; ++k) {
      const int yy = q.origin[1] + y;
      const int ys = (q.flip & 2) ? vol.H - 1 - yy : yy;
      off[k] = ((long long)zs * vol.H + ys) * vol.W + q.origin[2] + u;
      if (++u == w) { u = 0; ++y; }
    }
    float raw[4][AP_PER];
    unsigned char lab[AP_PER];
#pragma unroll
    for (int k = 0; k < AP_PER; ++k) {
      const long long o = k < cnt ? off[k] : off[0];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        raw[c][k] = f32 ? src_f((const float*)vol.img, c * DHW + o) : src_f((const short*)vol.img, c * DHW + o);
      lab[k] = vol.lab[o];
    }
#pragma unroll
    for (int k = 0; k < AP_PER; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float t = raw[c][k];
        if (do_scale) t = t * a_scale;
        if (do_shift && t != 0.f) t = t + shift_c[c];
        if (do_norm) t = t / 255.0f;                 // IEEE division (not a reciprocal product)
        xv[c][k] = t;
      }
      const unsigned l = lab[k];
      mv[0][k] = l > 0 ? 1.f : 0.f;
      mv[1][k] = (l >= 1 && l <= 3) ? 1.f : 0.f;
      mv[2][k] = l == 1 ? 1.f : 0.f;
    }
  }
  if (v4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) st4(xo, c * dhw, xv[c]);
#pragma unroll
    for (int j = 0; j < 3; ++j) st4(mo, j * dhw, mv[j]);
  } else {
    for (int k = 0; k < cnt; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) st_out(xo, c * dhw + k, xv[c][k]);
#pragma unroll
      for (int j = 0; j < 3; ++j) st_out(mo, j * dhw + k, mv[j][k]);
    }
  }
}

template <typename XT>
int aug_apply_m(hipStream_t st, dim3 grid, int m_dtype, const xh_aug_volume* vols, int nvol, const double* mom, const int* idx,
                const xh_aug_params* prm, int d, int h, int w, int flags, void* x, void* mask, bool vec) {
  XH_DISPATCH_T(m_dtype, hipLaunchKernelGGL((aug_apply_kernel<XT, T>), grid, dim3(AP_T), 0, st, vols, nvol, mom, idx, prm, d, h, w,
                                            flags, (XT*)x, (T*)mask, vec););
  return XH_OK;
}

int aug_apply_x(hipStream_t st, dim3 grid, int x_dtype, int m_dtype, const xh_aug_volume* vols, int nvol, const double* mom,
                const int* idx, const xh_aug_params* prm, int d, int h, int w, int flags, void* x, void* mask, bool vec) {
  XH_DISPATCH_T(x_dtype, return aug_apply_m<T>(st, grid, m_dtype, vols, nvol, mom, idx, prm, d, h, w, flags, x, mask, vec););
  return XH_OK;
}

}  // namespace

extern "C" long long xh_aug_moments_workspace_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return -1;
  return 4ll * mom_blocks((long long)D * H * W) * 3 * (long long)sizeof(double);
}

extern "C" int xh_aug_moments(void* stream, const xh_aug_volume* vol, void* ws, long long ws_bytes, double* out) {
  if (!vol || !vol->img || !ws || !out || vol->D <= 0 || vol->H <= 0 || vol->W <= 0) return XH_ERR_ARG;
  if (vol->dtype != XH_F32 && vol->dtype != XH_I16) return XH_ERR_DTYPE;
  const long long n = (long long)vol->D * vol->H * vol->W;
  const int nb = mom_blocks(n);
  if (ws_bytes < xh_aug_moments_workspace_bytes(vol->D, vol->H, vol->W)) return XH_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  long long chunk = (n + nb - 1) / nb;
  chunk = (chunk + 7) / 8 * 8;
  const dim3 grid(nb, 4);
  if (vol->dtype == XH_F32) {
    if (n % 4 == 0 && ((uintptr_t)vol->img & 15) == 0)
      hipLaunchKernelGGL((aug_moments_partial_kernel<float, true>), grid, dim3(MOM_T), 0, st, (const float*)vol->img, n, chunk, part);
    else
      hipLaunchKernelGGL((aug_moments_partial_kernel<float, false>), grid, dim3(MOM_T), 0, st, (const float*)vol->img, n, chunk, part);
  } else {
    if (n % 8 == 0 && ((uintptr_t)vol->img & 15) == 0)
      hipLaunchKernelGGL((aug_moments_partial_kernel<short, true>), grid, dim3(MOM_T), 0, st, (const short*)vol->img, n, chunk, part);
    else
      hipLaunchKernelGGL((aug_moments_partial_kernel<short, false>), grid, dim3(MOM_T), 0, st, (const short*)vol->img, n, chunk, part);
  }
  hipLaunchKernelGGL(aug_moments_final_kernel, dim3(4), dim3(MOM_T), 0, st, (const double*)part, nb, out);
  return xh_launch_status();
}

extern "C" int xh_aug_draw(void* stream, const xh_aug_volume* vols, int nvol, const int* idx, int N, const int* crop, int flags,
                           double s_scale, double s_shift, double flip_prob, unsigned long long* rng, xh_aug_params* params) {
  if (!vols || nvol <= 0 || !idx || N <= 0 || !crop || !rng || !params) return XH_ERR_ARG;
  if (crop[0] <= 0 || crop[1] <= 0 || crop[2] <= 0) return XH_ERR_ARG;
  hipLaunchKernelGGL(aug_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, vols, nvol, idx, N, crop[0], crop[1], crop[2], flags,
                     s_scale, s_shift, flip_prob, rng, params);
  return xh_launch_status();
}

extern "C" int xh_aug_apply(void* stream, const xh_aug_volume* vols, int nvol, const double* moments, const int* idx,
                            const xh_aug_params* params, int N, int d, int h, int w, int flags, int x_dtype, void* x, int m_dtype,
                            void* mask) {
  if (!vols || nvol <= 0 || !moments || !idx || !params || !x || !mask) return XH_ERR_ARG;
  if (N <= 0 || N > 65535 || d <= 0 || d > 65535 || h <= 0 || w <= 0 || (long long)h * w > (1ll << 30)) return XH_ERR_ARG;
  const long long hw = (long long)h * w;
  // 4-wide stores need every thread's first voxel 4-aligned in every channel plane: hw % 4 == 0 (outputs are contiguous)
  const bool vec = hw % AP_PER == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)mask & 15) == 0;
  const dim3 grid((unsigned)((hw + AP_TILE - 1) / AP_TILE), d, N);
  const int rc = aug_apply_x((hipStream_t)stream, grid, x_dtype, m_dtype, vols, nvol, moments, idx, params, d, h, w, flags, x, mask, vec);
  if (rc != XH_OK) return rc;
  return xh_launch_status();
}
