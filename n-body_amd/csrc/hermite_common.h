// hermite_common.h -- what the shared-step Hermite integrator (hermite.hip), the block-time-step one (hermite_block.hip)
// and its ensemble form (hermite_batch.hip) share: the pair bodies of the force-and-jerk sweep and its tile body, the
// launch shape, the predictor and corrector expressions and the two reductions of the finalize pass.  One definition
// each, with the state precision as a template flag (EXT), so that a block-step run whose bodies all sit on level 0
// rounds exactly as the shared-step run does, an extended run with zero residuals as an fp32 one, and system s of an
// ensemble as the single-system run.
#pragma once

#include <cmath>
#include <type_traits>

#include "common.h"

namespace nbh {

constexpr int TS = 256;  // sources per LDS tile (direct.hip)
static_assert(TS == kDirectTile, "direct_plan.h counts the source splits in tiles of TS");

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }

// ---------------------------------------------------------------------------------
// The pair bodies.  EXT: EXTENDED STATE PRECISION (double-single positions).  A body's position
// is hi + lo, two fp32 numbers, and the separation is d = (hi_j - hi_i) + (lo_j - lo_i) in fp32, in that association: the
// hi difference is exact for close pairs (Sterbenz), so d keeps the digits that fl(x_j) - fl(x_i) loses.  w comes from the
// hi parts of the velocities only.  The residuals (sl, lxi, lyi, lzi) are read under `if constexpr (EXT)` and nowhere
// else; everything after d and w is one text, so with all residuals zero the sums of the two forms are equal bit for bit.
// ---------------------------------------------------------------------------------
// One source against R targets, scalar form with the coincident-pair guard (eps2 < 1e-12).
template <int R, bool EXT>
__device__ __forceinline__ void jerk_guard(const float4 s, const float4 sv, const float4 sl, const float (&xi)[R],
                                           const float (&yi)[R], const float (&zi)[R], const float (&ui)[R],
                                           const float (&vi)[R], const float (&wi)[R], const float (&lxi)[R],
                                           const float (&lyi)[R], const float (&lzi)[R], float (&ax)[R], float (&ay)[R],
                                           float (&az)[R], float (&jx)[R], float (&jy)[R], float (&jz)[R],
                                           const float eps2) {
#pragma unroll
  for (int r = 0; r < R; r++) {
    float dx = s.x - xi[r], dy = s.y - yi[r], dz = s.z - zi[r];
    if constexpr (EXT) {
      dx += sl.x - lxi[r]; dy += sl.y - lyi[r]; dz += sl.z - lzi[r];
    }
    const float wx = sv.x - ui[r], wy = sv.y - vi[r], wz = sv.z - wi[r];
    const float d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    const float dw = __builtin_fmaf(dx, wx, __builtin_fmaf(dy, wy, dz * wz));
    // (rsq(0) = inf, and 0 * inf is not 0.  EXT, hi parts equal and lo parts not: a distinct pair, d2 > 0)
    const float inv = d2 > 0.0f ? rsq(d2 + eps2) : 0.0f;
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
// (m inv^3), 2 mul (-3 d.w inv^2), 3 fma (w + q d), 3 + 3 fma (sums) = 26 VALU + 1 transcendental.  EXT: 3 sub + 3 add
// more in the first phase, 32 + 1.
template <int R, int NS, bool EXT>
__device__ __forceinline__ void jerk_pk(const float4 (&s)[NS], const float4 (&sv)[NS], const float4 (&sl)[NS],
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
#pragma unroll
    for (int r = 0; r < H; r++) {
      const int c = k * H + r;
      dx[c] = sx - xi[r]; dy[c] = sy - yi[r]; dz[c] = sz - zi[r];
      if constexpr (EXT) {
        const f2 lx = {sl[k].x, sl[k].x}, ly = {sl[k].y, sl[k].y}, lz = {sl[k].z, sl[k].z};
        dx[c] += lx - lxi[r]; dy[c] += ly - lyi[r]; dz[c] += lz - lzi[r];
      }
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
// The tile body of the tiled sweep: the one text direct_jerk_kernel (hermite.hip: the shared step, the standalone
// evaluation, the wide form of the block scheme) and batch_prime_sweep_kernel (hermite_batch.hip) run per LDS tile, which
// is the whole of the bit equality between those forms.
// ---------------------------------------------------------------------------------
// The R targets of one lane ({xp, m} -> xi, yi, zi; {vp, 0} -> ui, vi, wi; EXT, {xp_lo, 0} -> lxi, lyi, lzi) against one
// LDS tile of TS sources in index order (padded sources: m = 0, at rest at the origin, residual 0): fp32 sums over the
// tile, folded into the lane's fp64 sums sa, sj.  GUARD: the scalar body, else the targets are packed in pairs and the
// packed body takes NS sources per call, so that R/2 * NS = 2 chains are in flight.  tile_l and the residuals of the
// targets are read in the EXT forms only.
// (The targets are plain arrays, the zeroes of the callers are written out where they are used: with the targets in a
// struct, or with one shared zero constant, the compiler vectorised the guarded forms another way and they lost a
// wave or two of occupancy.  The fp32 non-gathered instantiations of direct_jerk_kernel keep this text written out in
// the kernel, the one exception that the timing against the parent left: hermite.hip)
template <int R, bool GUARD, bool EXT>
__device__ __forceinline__ void jerk_tile(const float4* tile_p, const float4* tile_v, const float4* tile_l,
                                          const float (&xi)[R], const float (&yi)[R], const float (&zi)[R],
                                          const float (&ui)[R], const float (&vi)[R], const float (&wi)[R],
                                          const float (&lxi)[R], const float (&lyi)[R], const float (&lzi)[R],
                                          double (&sa)[3][R], double (&sj)[3][R], const float eps2) {
  if constexpr (!GUARD) {
    constexpr int H = R / 2;
    f2 px[H], py[H], pz[H], pu[H], pv[H], pw[H], lx[H], ly[H], lz[H], ax[H], ay[H], az[H], jx[H], jy[H], jz[H];
#pragma unroll
    for (int r = 0; r < H; r++) {
      px[r] = f2{xi[2 * r], xi[2 * r + 1]}; py[r] = f2{yi[2 * r], yi[2 * r + 1]}; pz[r] = f2{zi[2 * r], zi[2 * r + 1]};
      pu[r] = f2{ui[2 * r], ui[2 * r + 1]}; pv[r] = f2{vi[2 * r], vi[2 * r + 1]}; pw[r] = f2{wi[2 * r], wi[2 * r + 1]};
      lx[r] = f2{lxi[2 * r], lxi[2 * r + 1]}; ly[r] = f2{lyi[2 * r], lyi[2 * r + 1]}; lz[r] = f2{lzi[2 * r], lzi[2 * r + 1]};
      ax[r] = ay[r] = az[r] = jx[r] = jy[r] = jz[r] = f2{0.f, 0.f};
    }
    constexpr int NS = R >= 4 ? 1 : 2;
#pragma unroll 4
    for (int k = 0; k < TS; k += NS) {
      float4 sp[NS], sv[NS], sl[NS];
#pragma unroll
      for (int q = 0; q < NS; q++) {
        sp[q] = tile_p[k + q];
        sv[q] = tile_v[k + q];
        if constexpr (EXT) sl[q] = tile_l[k + q];
      }
      jerk_pk<R, NS, EXT>(sp, sv, sl, px, py, pz, pu, pv, pw, lx, ly, lz, ax, ay, az, jx, jy, jz, eps2);
    }
#pragma unroll
    for (int r = 0; r < H; r++) {
      sa[0][2 * r] += (double)ax[r].x; sa[0][2 * r + 1] += (double)ax[r].y;
      sa[1][2 * r] += (double)ay[r].x; sa[1][2 * r + 1] += (double)ay[r].y;
      sa[2][2 * r] += (double)az[r].x; sa[2][2 * r + 1] += (double)az[r].y;
      sj[0][2 * r] += (double)jx[r].x; sj[0][2 * r + 1] += (double)jx[r].y;
      sj[1][2 * r] += (double)jy[r].x; sj[1][2 * r + 1] += (double)jy[r].y;
      sj[2][2 * r] += (double)jz[r].x; sj[2][2 * r + 1] += (double)jz[r].y;
    }
  } else {
    float ax[R], ay[R], az[R], jx[R], jy[R], jz[R];
#pragma unroll
    for (int r = 0; r < R; r++) ax[r] = ay[r] = az[r] = jx[r] = jy[r] = jz[r] = 0.f;
#pragma unroll 4
    for (int k = 0; k < TS; k++) {
      float4 sl = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (EXT) sl = tile_l[k];
      jerk_guard<R, EXT>(tile_p[k], tile_v[k], sl, xi, yi, zi, ui, vi, wi, lxi, lyi, lzi, ax, ay, az, jx, jy, jz, eps2);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      sa[0][r] += (double)ax[r]; sa[1][r] += (double)ay[r]; sa[2][r] += (double)az[r];
      sj[0][r] += (double)jx[r]; sj[1][r] += (double)jy[r]; sj[2][r] += (double)jz[r];
    }
  }
}

struct HermiteArrays {
  float *x, *y, *z, *vx, *vy, *vz, *ax, *ay, *az, *aox, *aoy, *aoz;
};

// The fp32 residuals of the extended state, on the integrator's handle: X = pos + lo.x/y/z, V = vel + lo.vx/vy/vz, with
// hi = (float)X and lo = (float)(X - hi) after every call (24 bytes per body).  The fp32 forms (EXT = false) are handed
// HermiteLo{} and never read it.
struct HermiteLo {
  float *x, *y, *z, *vx, *vy, *vz;
};

// fp64 -> hi + lo: hi = (float)v, lo = (float)(v - hi); v - hi is exact, lo carries 24 more bits (error <= 2^-49 |v|)
__device__ __forceinline__ void split_f64(const double v, float& hi, float& lo) {
  hi = (float)v;
  lo = (float)(v - (double)hi);
}

// One component of body i's state in fp64: the fp32 number, or (EXT) hi + lo, an exact sum
template <bool EXT>
__device__ __forceinline__ double state_f64(const float* hi, const float* lo, const int i) {
  if constexpr (EXT) return (double)hi[i] + (double)lo[i];
  else return (double)hi[i];
}

// v rounded to what the state holds: fp32 (lo is not written), or (EXT) hi + lo
template <bool EXT>
__device__ __forceinline__ void round_state(const double v, float& hi, float& lo) {
  if constexpr (EXT) split_f64(v, hi, lo);
  else hi = (float)v;
}

// the value such a pair stands for
template <bool EXT>
__device__ __forceinline__ double state_f64(const float hi, const float lo) {
  if constexpr (EXT) return (double)hi + (double)lo;
  else return (double)hi;
}

// Predictor of body i over h, in fp64 from the state and rounded once: -> {xp, m}, {vp, 0}.  EXT: the same expressions
// on X = hi + lo and V = hi + lo, xp rounded to hi + lo -> {xp_hi, m}, {vp_hi, 0}, {xp_lo, 0}; the pair sweep takes no
// velocity residual.  fp32: lo and plo are not touched.
template <bool EXT>
__device__ __forceinline__ void hermite_predict(const double h, const float* __restrict__ x, const float* __restrict__ y,
                                                const float* __restrict__ z, const float* __restrict__ vx,
                                                const float* __restrict__ vy, const float* __restrict__ vz,
                                                const float* __restrict__ ax, const float* __restrict__ ay,
                                                const float* __restrict__ az, const float* __restrict__ m,
                                                const HermiteLo& lo, const float4* __restrict__ jerk, const int i,
                                                float4* __restrict__ posm, float4* __restrict__ vel,
                                                float4* __restrict__ plo) {
  const double h2 = 0.5 * h * h, h3 = h * h * h / 6.0;
  const float4 j = jerk[i];
  const double px = state_f64<EXT>(x, lo.x, i), py = state_f64<EXT>(y, lo.y, i), pz = state_f64<EXT>(z, lo.z, i);
  const double ux = state_f64<EXT>(vx, lo.vx, i), uy = state_f64<EXT>(vy, lo.vy, i), uz = state_f64<EXT>(vz, lo.vz, i);
  const double bx = ax[i], by = ay[i], bz = az[i];
  float hx, hy, hz, lx, ly, lz;
  round_state<EXT>(px + ux * h + bx * h2 + (double)j.x * h3, hx, lx);
  round_state<EXT>(py + uy * h + by * h2 + (double)j.y * h3, hy, ly);
  round_state<EXT>(pz + uz * h + bz * h2 + (double)j.z * h3, hz, lz);
  posm[i] = make_float4(hx, hy, hz, m[i]);
  if constexpr (EXT) plo[i] = make_float4(lx, ly, lz, 0.f);
  vel[i] = make_float4((float)(ux + bx * h + (double)j.x * h2), (float)(uy + by * h + (double)j.y * h2),
                       (float)(uz + bz * h + (double)j.z * h2), 0.f);
}

// Corrector of body i over h from the new (a1, j1) and the old jerk jerk[i] (fp64 from the fp32 state, rounded once):
// v <- v1, x <- x1, acc_old <- a, acc <- a1.  The caller stores j1.  EXT: v1 from V = hi + lo, rounded to hi + lo; x1
// from X, V and that v1, rounded to hi + lo; a and j stay fp32.  The one corrector of every form: the shared step's
// finalize pass, the block scheme's, the resident block step.
template <bool EXT>
__device__ __forceinline__ void hermite_correct(const double h, const HermiteArrays& d, const HermiteLo& lo, const int i,
                                                const float4* __restrict__ jerk, const float a1x, const float a1y,
                                                const float a1z, const float j1x, const float j1y, const float j1z) {
  const double hh = 0.5 * h, h12 = h * h / 12.0;
  const float4 j0 = jerk[i];
  const double a0x = d.ax[i], a0y = d.ay[i], a0z = d.az[i];
  const double v0x = state_f64<EXT>(d.vx, lo.vx, i), v0y = state_f64<EXT>(d.vy, lo.vy, i),
               v0z = state_f64<EXT>(d.vz, lo.vz, i);
  float vhx, vhy, vhz, vlx, vly, vlz, xh, xl;
  round_state<EXT>(v0x + (a0x + (double)a1x) * hh + ((double)j0.x - (double)j1x) * h12, vhx, vlx);
  round_state<EXT>(v0y + (a0y + (double)a1y) * hh + ((double)j0.y - (double)j1y) * h12, vhy, vly);
  round_state<EXT>(v0z + (a0z + (double)a1z) * hh + ((double)j0.z - (double)j1z) * h12, vhz, vlz);
  round_state<EXT>(state_f64<EXT>(d.x, lo.x, i) + (v0x + state_f64<EXT>(vhx, vlx)) * hh + (a0x - (double)a1x) * h12, xh, xl);
  d.x[i] = xh;
  if constexpr (EXT) lo.x[i] = xl;
  round_state<EXT>(state_f64<EXT>(d.y, lo.y, i) + (v0y + state_f64<EXT>(vhy, vly)) * hh + (a0y - (double)a1y) * h12, xh, xl);
  d.y[i] = xh;
  if constexpr (EXT) lo.y[i] = xl;
  round_state<EXT>(state_f64<EXT>(d.z, lo.z, i) + (v0z + state_f64<EXT>(vhz, vlz)) * hh + (a0z - (double)a1z) * h12, xh, xl);
  d.z[i] = xh;
  if constexpr (EXT) lo.z[i] = xl;
  d.vx[i] = vhx; d.vy[i] = vhy; d.vz[i] = vhz;
  if constexpr (EXT) {
    lo.vx[i] = vlx; lo.vy[i] = vly; lo.vz[i] = vlz;
  }
  d.aox[i] = (float)a0x; d.aoy[i] = (float)a0y; d.aoz[i] = (float)a0z;
  d.ax[i] = a1x; d.ay[i] = a1y; d.az[i] = a1z;
}

// a1 = G sum_splits pa, j1 = G sum_splits pj of row k of [splits][n_pad]: fp64, split order, G in fp64, rounded to fp32
__device__ __forceinline__ void jerk_sum_splits(const float4* __restrict__ pa, const float4* __restrict__ pj,
                                                const int splits, const int n_pad, const int k, const float G,
                                                float (&a1)[3], float (&j1)[3]) {
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < splits; q++) {
    const float4 p = pa[(size_t)q * n_pad + k], r = pj[(size_t)q * n_pad + k];
    s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z;
    s[3] += (double)r.x; s[4] += (double)r.y; s[5] += (double)r.z;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    a1[c] = (float)((double)G * s[c]);
    j1[c] = (float)((double)G * s[3 + c]);
  }
}

// the minimum of `ratio` over a block of kBlock threads folded into *hint: one atomicMin per block on the
// order-preserving integer (as the bounding-box reduction does; a min does not depend on the order of its operands)
__device__ __forceinline__ void block_min_ratio(float ratio, unsigned int* __restrict__ hint) {
  __shared__ float red[kBlock / kWave];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ratio = fminf(ratio, __shfl_down(ratio, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ratio;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = red[0];
#pragma unroll
    for (int k = 1; k < kBlock / kWave; k++) v = fminf(v, red[k]);
    if (v < INFINITY) atomicMin(hint, float_to_ordered(v));
  }
}

// (the launch shape of the one-sided force-and-jerk sweep, n_targets against n_sources: one_sided_shape of direct_plan.h
// without tuning, as nbody_hip_direct_field takes it)

inline bool finite_f(float v) { return v - v == 0.0f; }

// hermite.hip: the argument checks of the Hermite entry points, and one evaluation at the state (x, v) advanced by the
// predictor over dt (0: at the state itself) followed by the finalize pass.  Both null: fp32 state.  lo: extended state
// precision, the handle's residuals.  lo4 (given instead of lo by the standalone extended evaluation, which cannot
// correct): {lx, ly, lz, 0} per body on the device.
int hermite_check_arrays(const nbody_hip_ctx* ctx, const nbody_particle_data* d, bool need_old);
int hermite_evaluate(nbody_hip_ctx* ctx, const nbody_particle_data* d, const HermiteLo* lo, const float4* lo4, float G,
                     float eps, float dt, int correct, const float4* jerk_in, float4* acc4, float4* jerk_out,
                     unsigned int* hint);
// the wide sweep (direct_jerk_kernel): n_targets targets (list == nullptr: the bodies themselves, n_targets == n; else
// gathered through list) against the n predicted sources {posm, vel} and, extended state precision, plo (else nullptr)
void hermite_launch_jerk(const nbody_hip_ctx* ctx, const OneSidedShape& s, bool guard, const float4* posm, const float4* vel,
                         const float4* plo, const int* list, int n_targets, int n, float4* pa, float4* pj, float eps2);
// host side of set / get_state_f64 and of the residual storage (allocated at first use, zeroed on the context's stream),
// shared by the two handles
int hermite_lo_zero(nbody_hip_ctx* ctx, size_t max_particles, float** mem, HermiteLo* lo);
int hermite_state_set_f64(nbody_hip_ctx* ctx, nbody_particle_data* d, const HermiteLo* lo_or_null, const double* pos,
                          const double* vel);
int hermite_state_get_f64(nbody_hip_ctx* ctx, const nbody_particle_data* d, const HermiteLo* lo_or_null, double* pos,
                          double* vel);

}  // namespace nbh
