// hermite_common.h -- what the shared-step Hermite integrator (hermite.hip) and the block-time-step one
// (hermite_block.hip) share: the pair bodies of the force-and-jerk sweep, its launch shape, and the predictor and
// corrector expressions.  One definition each, so that a block-step run whose bodies all sit on level 0 rounds exactly
// as the shared-step run does.
#pragma once

#include "common.h"

namespace nbh {

constexpr int TS = 256;  // sources per LDS tile (direct.hip)

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }

// ---------------------------------------------------------------------------------
// One source against R targets, scalar form with the coincident-pair guard (eps2 < 1e-12).
// ---------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void jerk_guard(const float4 s, const float4 sv, const float (&xi)[R], const float (&yi)[R],
                                           const float (&zi)[R], const float (&ui)[R], const float (&vi)[R],
                                           const float (&wi)[R], float (&ax)[R], float (&ay)[R], float (&az)[R],
                                           float (&jx)[R], float (&jy)[R], float (&jz)[R], const float eps2) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    const float dx = s.x - xi[r], dy = s.y - yi[r], dz = s.z - zi[r];
    const float wx = sv.x - ui[r], wy = sv.y - vi[r], wz = sv.z - wi[r];
    const float d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    const float dw = __builtin_fmaf(dx, wx, __builtin_fmaf(dy, wy, dz * wz));
    const float inv = d2 > 0.0f ? rsq(d2 + eps2) : 0.0f;  // (rsq(0) = inf, and 0 * inf is not 0)
    const float inv2 = inv * inv;
    const float f = (s.w * inv) * inv2;
    const float q = (dw * inv2) * -3.0f;
    ax[r] = __builtin_fmaf(f, dx, ax[r]);
    ay[r] = __builtin_fmaf(f, dy, ay[r]);
    az[r] = __builtin_fmaf(f, dz, az[r]);
    jx[r] = __builtin_fmaf(f, __builtin_fmaf(q, dx, wx), jx[r]);
    jy[r] = __builtin_fmaf(f, __builtin_fmaf(q, dy, wy), jy[r]);
    jz[r] = __builtin_fmaf(f, __builtin_fmaf(q, dz, wz), jz[r]);
  }
}

// Packed form: two targets per v_pk_*_f32 instruction, NS sources per call, written in phases over the NS * R/2
// independent chains like interact_pk (direct.hip): all differences and both dot products, then every v_rsq_f32, then
// the factors, then the six sums.  Per pair: 6 sub, 3 fma (h), 1 mul + 2 fma (d.w), rsq, 1 mul (inv^2), 2 mul
// (m inv^3), 2 mul (-3 d.w inv^2), 3 fma (w + q d), 3 + 3 fma (sums) = 26 VALU + 1 transcendental.
template <int R, int NS>
__device__ __forceinline__ void jerk_pk(const float4 (&s)[NS], const float4 (&sv)[NS], const f2 (&xi)[R / 2],
                                        const f2 (&yi)[R / 2], const f2 (&zi)[R / 2], const f2 (&ui)[R / 2],
                                        const f2 (&vi)[R / 2], const f2 (&wi)[R / 2], f2 (&ax)[R / 2], f2 (&ay)[R / 2],
                                        f2 (&az)[R / 2], f2 (&jx)[R / 2], f2 (&jy)[R / 2], f2 (&jz)[R / 2],
                                        const float eps2) {
  constexpr int H = R / 2;
  const f2 e2 = {eps2, eps2};
  const f2 m3 = {-3.0f, -3.0f};
  f2 dx[NS * H], dy[NS * H], dz[NS * H], wx[NS * H], wy[NS * H], wz[NS * H], g[NS * H], q[NS * H];
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const f2 sx = {s[k].x, s[k].x}, sy = {s[k].y, s[k].y}, sz = {s[k].z, s[k].z};
    const f2 su = {sv[k].x, sv[k].x}, sw = {sv[k].y, sv[k].y}, st = {sv[k].z, sv[k].z};
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      dx[c] = sx - xi[r]; dy[c] = sy - yi[r]; dz[c] = sz - zi[r];
      wx[c] = su - ui[r]; wy[c] = sw - vi[r]; wz[c] = st - wi[r];
      g[c] = __builtin_elementwise_fma(dx[c], dx[c], __builtin_elementwise_fma(dy[c], dy[c], __builtin_elementwise_fma(dz[c], dz[c], e2)));
      q[c] = __builtin_elementwise_fma(dx[c], wx[c], __builtin_elementwise_fma(dy[c], wy[c], dz[c] * wz[c]));
    }
  }
#pragma unroll
  for (int c = 0; c < NS * H; c++) {
    g[c].x = rsq(g[c].x);
    g[c].y = rsq(g[c].y);
  }
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const f2 sm = {s[k].w, s[k].w};
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      const f2 inv2 = g[c] * g[c];
      g[c] = (sm * g[c]) * inv2;   // f = m inv^3: the chain of interact_pk
      q[c] = (q[c] * inv2) * m3;   // -3 (d.w) / h
      wx[c] = __builtin_elementwise_fma(q[c], dx[c], wx[c]);
      wy[c] = __builtin_elementwise_fma(q[c], dy[c], wy[c]);
      wz[c] = __builtin_elementwise_fma(q[c], dz[c], wz[c]);
    }
  }
#pragma unroll
  for (int k = 0; k < NS; k++) {
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      ax[r] = __builtin_elementwise_fma(g[c], dx[c], ax[r]);
      ay[r] = __builtin_elementwise_fma(g[c], dy[c], ay[r]);
      az[r] = __builtin_elementwise_fma(g[c], dz[c], az[r]);
      jx[r] = __builtin_elementwise_fma(g[c], wx[c], jx[r]);
      jy[r] = __builtin_elementwise_fma(g[c], wy[c], jy[r]);
      jz[r] = __builtin_elementwise_fma(g[c], wz[c], jz[r]);
    }
  }
}

// ---------------------------------------------------------------------------------
// EXTENDED STATE PRECISION (double-single positions in the pair sweep).  A body's position is
// hi + lo, two fp32 numbers; the separation is d = (hi_j - hi_i) + (lo_j - lo_i) in fp32, in that association: the hi
// difference is exact for close pairs (Sterbenz), so d keeps the digits that fl(x_j) - fl(x_i) loses.  w comes from the hi
// parts of the velocities only.  Everything after d and w is the body above, operation for operation: with all
// residuals zero the sums are those of jerk_guard / jerk_pk bit for bit.
// ---------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void jerk_guard_ext(const float4 s, const float4 sv, const float4 sl, const float (&xi)[R],
                                               const float (&yi)[R], const float (&zi)[R], const float (&ui)[R],
                                               const float (&vi)[R], const float (&wi)[R], const float (&lxi)[R],
                                               const float (&lyi)[R], const float (&lzi)[R], float (&ax)[R],
                                               float (&ay)[R], float (&az)[R], float (&jx)[R], float (&jy)[R],
                                               float (&jz)[R], const float eps2) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    const float dx = (s.x - xi[r]) + (sl.x - lxi[r]), dy = (s.y - yi[r]) + (sl.y - lyi[r]),
                dz = (s.z - zi[r]) + (sl.z - lzi[r]);
    const float wx = sv.x - ui[r], wy = sv.y - vi[r], wz = sv.z - wi[r];
    const float d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    const float dw = __builtin_fmaf(dx, wx, __builtin_fmaf(dy, wy, dz * wz));
    const float inv = d2 > 0.0f ? rsq(d2 + eps2) : 0.0f;  // (hi parts equal, lo parts not: a distinct pair, d2 > 0)
    const float inv2 = inv * inv;
    const float f = (s.w * inv) * inv2;
    const float q = (dw * inv2) * -3.0f;
    ax[r] = __builtin_fmaf(f, dx, ax[r]);
    ay[r] = __builtin_fmaf(f, dy, ay[r]);
    az[r] = __builtin_fmaf(f, dz, az[r]);
    jx[r] = __builtin_fmaf(f, __builtin_fmaf(q, dx, wx), jx[r]);
    jy[r] = __builtin_fmaf(f, __builtin_fmaf(q, dy, wy), jy[r]);
    jz[r] = __builtin_fmaf(f, __builtin_fmaf(q, dz, wz), jz[r]);
  }
}

// jerk_pk with the residuals: per pair 3 sub + 3 add more in the first phase, 32 packed-equivalent VALU + 1
// transcendental against 26 + 1.
template <int R, int NS>
__device__ __forceinline__ void jerk_pk_ext(const float4 (&s)[NS], const float4 (&sv)[NS], const float4 (&sl)[NS],
                                            const f2 (&xi)[R / 2], const f2 (&yi)[R / 2], const f2 (&zi)[R / 2],
                                            const f2 (&ui)[R / 2], const f2 (&vi)[R / 2], const f2 (&wi)[R / 2],
                                            const f2 (&lxi)[R / 2], const f2 (&lyi)[R / 2], const f2 (&lzi)[R / 2],
                                            f2 (&ax)[R / 2], f2 (&ay)[R / 2], f2 (&az)[R / 2], f2 (&jx)[R / 2],
                                            f2 (&jy)[R / 2], f2 (&jz)[R / 2], const float eps2) {
  constexpr int H = R / 2;
  const f2 e2 = {eps2, eps2};
  const f2 m3 = {-3.0f, -3.0f};
  f2 dx[NS * H], dy[NS * H], dz[NS * H], wx[NS * H], wy[NS * H], wz[NS * H], g[NS * H], q[NS * H];
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const f2 sx = {s[k].x, s[k].x}, sy = {s[k].y, s[k].y}, sz = {s[k].z, s[k].z};
    const f2 su = {sv[k].x, sv[k].x}, sw = {sv[k].y, sv[k].y}, st = {sv[k].z, sv[k].z};
    const f2 lx = {sl[k].x, sl[k].x}, ly = {sl[k].y, sl[k].y}, lz = {sl[k].z, sl[k].z};
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      dx[c] = (sx - xi[r]) + (lx - lxi[r]); dy[c] = (sy - yi[r]) + (ly - lyi[r]); dz[c] = (sz - zi[r]) + (lz - lzi[r]);
      wx[c] = su - ui[r]; wy[c] = sw - vi[r]; wz[c] = st - wi[r];
      g[c] = __builtin_elementwise_fma(dx[c], dx[c], __builtin_elementwise_fma(dy[c], dy[c], __builtin_elementwise_fma(dz[c], dz[c], e2)));
      q[c] = __builtin_elementwise_fma(dx[c], wx[c], __builtin_elementwise_fma(dy[c], wy[c], dz[c] * wz[c]));
    }
  }
#pragma unroll
  for (int c = 0; c < NS * H; c++) {
    g[c].x = rsq(g[c].x);
    g[c].y = rsq(g[c].y);
  }
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const f2 sm = {s[k].w, s[k].w};
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      const f2 inv2 = g[c] * g[c];
      g[c] = (sm * g[c]) * inv2;
      q[c] = (q[c] * inv2) * m3;
      wx[c] = __builtin_elementwise_fma(q[c], dx[c], wx[c]);
      wy[c] = __builtin_elementwise_fma(q[c], dy[c], wy[c]);
      wz[c] = __builtin_elementwise_fma(q[c], dz[c], wz[c]);
    }
  }
#pragma unroll
  for (int k = 0; k < NS; k++) {
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      ax[r] = __builtin_elementwise_fma(g[c], dx[c], ax[r]);
      ay[r] = __builtin_elementwise_fma(g[c], dy[c], ay[r]);
      az[r] = __builtin_elementwise_fma(g[c], dz[c], az[r]);
      jx[r] = __builtin_elementwise_fma(g[c], wx[c], jx[r]);
      jy[r] = __builtin_elementwise_fma(g[c], wy[c], jy[r]);
      jz[r] = __builtin_elementwise_fma(g[c], wz[c], jz[r]);
    }
  }
}

struct HermiteArrays {
  float *x, *y, *z, *vx, *vy, *vz, *ax, *ay, *az, *aox, *aoy, *aoz;
};

// Predictor of body i over h (fp64 from the fp32 state, rounded once): -> {xp, m}, {vp, 0}.
__device__ __forceinline__ void hermite_predict(const double h, const float* __restrict__ x, const float* __restrict__ y,
                                                const float* __restrict__ z, const float* __restrict__ vx,
                                                const float* __restrict__ vy, const float* __restrict__ vz,
                                                const float* __restrict__ ax, const float* __restrict__ ay,
                                                const float* __restrict__ az, const float* __restrict__ m,
                                                const float4* __restrict__ jerk, const int i, float4* __restrict__ posm,
                                                float4* __restrict__ vel) {
  const double h2 = 0.5 * h * h, h3 = h * h * h / 6.0;
  const float4 j = jerk[i];
  const double px = x[i], py = y[i], pz = z[i], ux = vx[i], uy = vy[i], uz = vz[i];
  const double bx = ax[i], by = ay[i], bz = az[i];
  posm[i] = make_float4((float)(px + ux * h + bx * h2 + (double)j.x * h3), (float)(py + uy * h + by * h2 + (double)j.y * h3),
                        (float)(pz + uz * h + bz * h2 + (double)j.z * h3), m[i]);
  vel[i] = make_float4((float)(ux + bx * h + (double)j.x * h2), (float)(uy + by * h + (double)j.y * h2),
                       (float)(uz + bz * h + (double)j.z * h2), 0.f);
}

// Corrector of body i over h from the new (a1, j1) and the old jerk jerk[i] (fp64 from the fp32 state, rounded once):
// v <- v1, x <- x1, acc_old <- a, acc <- a1.  The caller stores j1.  The expressions of hermite_finalize_kernel, which
// keeps its own copy: routed through this function its instruction stream changed (register allocation only).
__device__ __forceinline__ void hermite_correct(const double h, const HermiteArrays& d, const int i,
                                                const float4* __restrict__ jerk, const float a1x, const float a1y, const float a1z, const float j1x,
                                                const float j1y, const float j1z) {
  const double hh = 0.5 * h, h12 = h * h / 12.0;
  const float4 j0 = jerk[i];
  const double a0x = d.ax[i], a0y = d.ay[i], a0z = d.az[i];
  const double v0x = d.vx[i], v0y = d.vy[i], v0z = d.vz[i];
  const float v1x = (float)(v0x + (a0x + (double)a1x) * hh + ((double)j0.x - (double)j1x) * h12);
  const float v1y = (float)(v0y + (a0y + (double)a1y) * hh + ((double)j0.y - (double)j1y) * h12);
  const float v1z = (float)(v0z + (a0z + (double)a1z) * hh + ((double)j0.z - (double)j1z) * h12);
  d.x[i] = (float)((double)d.x[i] + (v0x + (double)v1x) * hh + (a0x - (double)a1x) * h12);
  d.y[i] = (float)((double)d.y[i] + (v0y + (double)v1y) * hh + (a0y - (double)a1y) * h12);
  d.z[i] = (float)((double)d.z[i] + (v0z + (double)v1z) * hh + (a0z - (double)a1z) * h12);
  d.vx[i] = v1x; d.vy[i] = v1y; d.vz[i] = v1z;
  d.aox[i] = (float)a0x; d.aoy[i] = (float)a0y; d.aoz[i] = (float)a0z;
  d.ax[i] = a1x; d.ay[i] = a1y; d.az[i] = a1z;
}

// The fp32 residuals of the extended state, on the integrator's handle: X = pos + lo.x/y/z, V = vel + lo.vx/vy/vz, with
// hi = (float)X and lo = (float)(X - hi) after every call (24 bytes per body).
struct HermiteLo {
  float *x, *y, *z, *vx, *vy, *vz;
};

// fp64 -> hi + lo: hi = (float)v, lo = (float)(v - hi); v - hi is exact, lo carries 24 more bits (error <= 2^-49 |v|)
__device__ __forceinline__ void split_f64(const double v, float& hi, float& lo) {
  hi = (float)v;
  lo = (float)(v - (double)hi);
}

// hermite_predict from the extended state: the same fp64 expressions on X = hi + lo and V = hi + lo (exact sums in
// fp64), xp rounded to hi + lo -> {xp_hi, m}, {vp_hi, 0}, {xp_lo, 0}.  The pair sweep takes no velocity residual.
__device__ __forceinline__ void hermite_predict_ext(const double h, const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ z, const float* __restrict__ vx,
                                                    const float* __restrict__ vy, const float* __restrict__ vz,
                                                    const float* __restrict__ ax, const float* __restrict__ ay,
                                                    const float* __restrict__ az, const float* __restrict__ m,
                                                    const HermiteLo& lo, const float4* __restrict__ jerk, const int i,
                                                    float4* __restrict__ posm, float4* __restrict__ vel,
                                                    float4* __restrict__ plo) {
  const double h2 = 0.5 * h * h, h3 = h * h * h / 6.0;
  const float4 j = jerk[i];
  const double px = (double)x[i] + (double)lo.x[i], py = (double)y[i] + (double)lo.y[i], pz = (double)z[i] + (double)lo.z[i];
  const double ux = (double)vx[i] + (double)lo.vx[i], uy = (double)vy[i] + (double)lo.vy[i],
               uz = (double)vz[i] + (double)lo.vz[i];
  const double bx = ax[i], by = ay[i], bz = az[i];
  float hx, hy, hz, lx, ly, lz;
  split_f64(px + ux * h + bx * h2 + (double)j.x * h3, hx, lx);
  split_f64(py + uy * h + by * h2 + (double)j.y * h3, hy, ly);
  split_f64(pz + uz * h + bz * h2 + (double)j.z * h3, hz, lz);
  posm[i] = make_float4(hx, hy, hz, m[i]);
  plo[i] = make_float4(lx, ly, lz, 0.f);
  vel[i] = make_float4((float)(ux + bx * h + (double)j.x * h2), (float)(uy + by * h + (double)j.y * h2),
                       (float)(uz + bz * h + (double)j.z * h2), 0.f);
}

// hermite_correct on the extended state: v1 in fp64 from V = hi + lo, rounded to hi + lo; x1 from X, V and that v1,
// rounded to hi + lo.  a and j stay fp32: acc_old <- a, acc <- a1; the caller stores j1.
__device__ __forceinline__ void hermite_correct_ext(const double h, const HermiteArrays& d, const HermiteLo& lo, const int i,
                                                    const float4* __restrict__ jerk, const float a1x, const float a1y,
                                                    const float a1z, const float j1x, const float j1y, const float j1z) {
  const double hh = 0.5 * h, h12 = h * h / 12.0;
  const float4 j0 = jerk[i];
  const double a0x = d.ax[i], a0y = d.ay[i], a0z = d.az[i];
  const double v0x = (double)d.vx[i] + (double)lo.vx[i], v0y = (double)d.vy[i] + (double)lo.vy[i],
               v0z = (double)d.vz[i] + (double)lo.vz[i];
  float vhx, vhy, vhz, vlx, vly, vlz, xh, xl;
  split_f64(v0x + (a0x + (double)a1x) * hh + ((double)j0.x - (double)j1x) * h12, vhx, vlx);
  split_f64(v0y + (a0y + (double)a1y) * hh + ((double)j0.y - (double)j1y) * h12, vhy, vly);
  split_f64(v0z + (a0z + (double)a1z) * hh + ((double)j0.z - (double)j1z) * h12, vhz, vlz);
  const double v1x = (double)vhx + (double)vlx, v1y = (double)vhy + (double)vly, v1z = (double)vhz + (double)vlz;
  split_f64((double)d.x[i] + (double)lo.x[i] + (v0x + v1x) * hh + (a0x - (double)a1x) * h12, xh, xl);
  d.x[i] = xh; lo.x[i] = xl;
  split_f64((double)d.y[i] + (double)lo.y[i] + (v0y + v1y) * hh + (a0y - (double)a1y) * h12, xh, xl);
  d.y[i] = xh; lo.y[i] = xl;
  split_f64((double)d.z[i] + (double)lo.z[i] + (v0z + v1z) * hh + (a0z - (double)a1z) * h12, xh, xl);
  d.z[i] = xh; lo.z[i] = xl;
  d.vx[i] = vhx; d.vy[i] = vhy; d.vz[i] = vhz;
  lo.vx[i] = vlx; lo.vy[i] = vly; lo.vz[i] = vlz;
  d.aox[i] = (float)a0x; d.aoy[i] = (float)a0y; d.aoz[i] = (float)a0z;
  d.ax[i] = a1x; d.ay[i] = a1y; d.az[i] = a1z;
}

// Launch shape of the one-sided force-and-jerk sweep, n_targets against n_sources: choose_shape's automatic one
// (direct.hip), as nbody_hip_direct_field takes it -- 4 targets per lane from 32,768 targets, else 2; source splits from
// the target count so that 256 CUs x 16 blocks are queued.
struct JerkShape { int R, splits, src_per_split, blocks_x, n_pad; };

inline JerkShape jerk_shape(size_t n_targets, size_t n_sources) {
  JerkShape s;
  s.R = n_targets >= 32768 ? 4 : 2;
  s.blocks_x = (int)((n_targets + (size_t)kBlock * s.R - 1) / ((size_t)kBlock * s.R));
  s.n_pad = s.blocks_x * kBlock * s.R;
  const int tiles = (int)((n_sources + TS - 1) / TS);
  int want = (kNumCU * 16 + s.blocks_x - 1) / s.blocks_x;
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  if (want > tiles) want = tiles > 0 ? tiles : 1;
  const int tiles_per_split = (tiles + want - 1) / want;
  s.src_per_split = tiles_per_split * TS;
  s.splits = (tiles + tiles_per_split - 1) / tiles_per_split;
  if (s.splits < 1) s.splits = 1;
  return s;
}
inline JerkShape jerk_shape(size_t n) { return jerk_shape(n, n); }

inline bool finite_f(float v) { return v - v == 0.0f; }

// hermite.hip: the argument checks of the Hermite entry points, and one evaluation at the state (x, v) advanced by the
// predictor over dt (0: at the state itself) followed by the finalize pass
int hermite_check_arrays(const nbody_hip_ctx* ctx, const nbody_particle_data* d, bool need_old);
int hermite_evaluate(nbody_hip_ctx* ctx, const nbody_particle_data* d, float G, float eps, float dt, int correct,
                     const float4* jerk_in, float4* acc4, float4* jerk_out, unsigned int* hint);
// the same in extended state precision.  lo: the handle's residuals; lo4 (given instead of lo by the standalone
// evaluation, which cannot correct): {lx, ly, lz, 0} per body on the device
int hermite_evaluate_ext(nbody_hip_ctx* ctx, const nbody_particle_data* d, const HermiteLo* lo, const float4* lo4, float G,
                         float eps, float dt, int correct, const float4* jerk_in, float4* acc4, float4* jerk_out,
                         unsigned int* hint);
// the extended wide sweep: n_targets targets (list == nullptr: the bodies themselves, n_targets == n; else gathered
// through list) against the n predicted sources {posm, vel, plo}
void hermite_launch_jerk_ext(const nbody_hip_ctx* ctx, const JerkShape& s, bool guard, const float4* posm,
                             const float4* vel, const float4* plo, const int* list, int n_targets, int n, float4* pa,
                             float4* pj, float eps2);
// host side of set / get_state_f64 and of the residual storage (allocated at first use, zeroed on the context's stream),
// shared by the two handles
int hermite_lo_zero(nbody_hip_ctx* ctx, size_t max_particles, float** mem, HermiteLo* lo);
int hermite_state_set_f64(nbody_hip_ctx* ctx, nbody_particle_data* d, const HermiteLo* lo_or_null, const double* pos,
                          const double* vel);
int hermite_state_get_f64(nbody_hip_ctx* ctx, const nbody_particle_data* d, const HermiteLo* lo_or_null, double* pos,
                          double* vel);

}  // namespace nbh
