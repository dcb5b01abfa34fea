// hermite.hip -- Direct N^2 force AND JERK for gfx950 (MI355X), and the fourth-order Hermite integrator on top of it
// (no reference counterpart: the reference integrates with Velocity Verlet only, src/cuda/integrator.cu:224-238).
//
// With d = r_j - r_i, w = v_j - v_i, h = |d|^2 + eps^2 (the softened pair kernel of direct.hip):
//     a_i = G sum_j m_j d h^-3/2
//     j_i = da_i/dt = G sum_j m_j [ w - 3 (d.w)/h d ] h^-3/2
// Conventions of direct_kernel, so that the a part forms the chain interact<> / interact_pk<> forms: no per-pair branch;
// the self pair (d = w = 0) contributes f * 0 = 0 to both sums; a coincident pair of two distinct bodies contributes 0 to
// a and m_j w / eps^3 to j (the derivative of the softened kernel); padded sources carry m = 0; eps^2 < 1e-12 takes the
// GUARD instantiation (d^2 = 0 => contribution 0 to both); per-tile fp32 sums are folded into fp64 every TS sources,
// source splits are added in fixed order in fp64 by the finalize pass, G is applied in fp64.  Nothing is summed with
// atomics: results are bitwise reproducible from call to call.
//
// One step of size dt is the PEC scheme of Makino & Aarseth (1992) as Hut & Makino write it, state in fp32:
//     xp = x + v dt + a dt^2/2 + j dt^3/6         vp = v + a dt + j dt^2/2                        (predict)
//     (a1, j1) = evaluate(xp, vp)                                                                 (one N^2 sweep)
//     v1 = v + (a + a1) dt/2 + (j - j1) dt^2/12   x1 = x + (v + v1) dt/2 + (a - a1) dt^2/12       (correct)
// Predictor and corrector are evaluated in fp64 from the fp32 state and rounded once.  After a step acc_* = a1 and
// acc_old_* = a (what the arrays mean after a Velocity-Verlet step); j1 lives on the integrator's handle.  a1 and j1 were
// evaluated at the PREDICTED state, as in every PEC Hermite code: a run continued from a checkpoint re-primes (a, j) at
// the corrected state, so continuation after save / load agrees to truncation order, NOT bit for bit (unlike the Direct
// Velocity-Verlet path).
//
// Three launches per step: hermite_predict_pack_kernel (SoA -> float4 {xp, m}, {vp, 0}), direct_jerk_kernel (the
// one-sided tiled shape of direct_kernel with two float4 per source), hermite_finalize_kernel (splits, G, corrector,
// min |a| / |j| for the time-step hint).  Roofline: FP32 VALU issue bound, 26 VALU + 1 transcendental per pair against
// 12 + 1 of the force kernel.
// The pair bodies, the tile body, the launch shape, the predictor and the corrector live in hermite_common.h.
//
// EXTENDED STATE PRECISION (opt-in, nbody_hip_hermite_set_precision): the state is X = pos + pos_lo,
// V = vel + vel_lo with fp32 residuals on the handle (24 bytes per body); predictor and corrector round to hi + lo
// instead of to fp32, and the sweep forms d = (hi_j - hi_i) + (lo_j - lo_i) from three float4 per source.  The three
// kernels are templates on the precision (EXT): one text each, what differs stands under `if constexpr (EXT)`; the host
// picks the instantiation, no kernel branches on it, and an fp32 instantiation neither reads a residual nor pays LDS
// or registers for one.  direct_jerk_kernel is also the wide sweep of the block scheme (hermite_block.hip), with its
// targets gathered through the active list (GATHER): hermite_launch_jerk is the one launcher, hermite_evaluate the one
// evaluation (predict, sweep, finalize) of the step, of both primings and of the standalone evaluations.

#include <cmath>
#include <cstring>
#include <vector>

#include "hermite_common.h"
#include "hermite_handle.h"

namespace nbh {

constexpr unsigned int kHintEmpty = 0xff800000u;  // float_to_ordered(+inf): no body with |j| > 0 seen

// ---------------------------------------------------------------------------------
// predict + pack: {xp, m}, {vp, 0} and, EXT, {xp_lo, 0}.  dt == 0 (priming, the standalone evaluation): the plain pack
// of the state (and its residuals), j is not read.
// One sweep: 13 (10) scalar loads and two 16-byte stores per body in fp32.  Re-arms the hint word for the finalize pass
// of the same evaluation (same stream, so ordered before it).
// ---------------------------------------------------------------------------------
template <bool EXT>
__global__ __launch_bounds__(kBlock) void hermite_predict_pack_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
    const float* __restrict__ vx, const float* __restrict__ vy, const float* __restrict__ vz,
    const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az,
    const float* __restrict__ m, HermiteLo lo, const float4* __restrict__ jerk, int n, float dt,
    float4* __restrict__ posm, float4* __restrict__ vel, float4* __restrict__ plo, unsigned int* __restrict__ hint) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) *hint = kHintEmpty;
  if (i >= n) return;
  if (dt == 0.0f) {
    posm[i] = make_float4(x[i], y[i], z[i], m[i]);
    vel[i] = make_float4(vx[i], vy[i], vz[i], 0.f);
    if constexpr (EXT) plo[i] = make_float4(lo.x[i], lo.y[i], lo.z[i], 0.f);
    return;
  }
  hermite_predict<EXT>((double)dt, x, y, z, vx, vy, vz, ax, ay, az, m, lo, jerk, i, posm, vel, plo);
}

// ---------------------------------------------------------------------------------
// Main kernel.  grid = (ceil(n_targets / (256 R)), splits); block = 256.  GATHER: the targets are list[0 .. n_targets)
// (the wide form of the block scheme), else the bodies themselves (n_targets == n; list is not read).
// pa[split][k] = {sum f dx, sum f dy, sum f dz, 0}, pj[split][k] = the jerk sums of target k over the split's sources,
// rounded to fp32 (G not applied).  Double-buffered LDS tiles of TS sources, two float4 per source (EXT: three, {xp_lo, 0}
// from plo; the fp32 forms neither read plo nor hold a third tile); one barrier per tile with the next tile's global loads
// in flight under the math (direct_kernel).  The tile itself is jerk_tile (hermite_common.h), which the fp32
// non-gathered instantiations keep written out (see there).
// ---------------------------------------------------------------------------------
template <int R, bool GUARD, bool EXT, bool GATHER>
__global__ __launch_bounds__(kBlock) void direct_jerk_kernel(const float4* __restrict__ posm,
                                                             const float4* __restrict__ vel,
                                                             const float4* __restrict__ plo,
                                                             const int* __restrict__ list, int n_targets, int n,
                                                             int src_per_split, float4* __restrict__ pa,
                                                             float4* __restrict__ pj, int n_pad, float eps2) {
  __shared__ float4 tile_p[2][TS];
  __shared__ float4 tile_v[2][TS];
  __shared__ float4 tile_l[2][EXT ? TS : 1];  // (fp32: a placeholder nothing touches)
  const int tid = threadIdx.x;
  const int tbase = blockIdx.x * (kBlock * R);

  float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R], lxi[R], lyi[R], lzi[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int k = tbase + r * kBlock + tid;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p, l = p;
    if (k < n_targets) {
      int i = k;
      if constexpr (GATHER) i = list[k];
      p = posm[i];
      v = vel[i];
      if constexpr (EXT) l = plo[i];
    }
    xi[r] = p.x; yi[r] = p.y; zi[r] = p.z;
    ui[r] = v.x; vi[r] = v.y; wi[r] = v.z;
    lxi[r] = l.x; lyi[r] = l.y; lzi[r] = l.z;
  }
  double sa[3][R], sj[3][R];
#pragma unroll
  for (int r = 0; r < R; r++) sa[0][r] = sa[1][r] = sa[2][r] = sj[0][r] = sj[1][r] = sj[2][r] = 0.0;

  const int j0 = blockIdx.y * src_per_split;
  const int j1 = min(n, j0 + src_per_split);
  const int ntiles = (j1 - j0 + TS - 1) / TS;
  // padded source: m = 0, at rest at the origin, residual 0
  float4 pre_p = make_float4(0.f, 0.f, 0.f, 0.f), pre_v = pre_p, pre_l = pre_p;
  if (j0 + tid < j1) {
    pre_p = posm[j0 + tid];
    pre_v = vel[j0 + tid];
    if constexpr (EXT) pre_l = plo[j0 + tid];
  }
  for (int it = 0; it < ntiles; it++) {
    const int b = it & 1;
    tile_p[b][tid] = pre_p;
    tile_v[b][tid] = pre_v;
    if constexpr (EXT) tile_l[b][tid] = pre_l;
    __syncthreads();  // one barrier per tile: the other buffer is only rewritten after the next barrier
    const int jn = j0 + (it + 1) * TS + tid;
    pre_p = pre_v = pre_l = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jn < j1) {  // next tile in flight under the math
      pre_p = posm[jn];
      pre_v = vel[jn];
      if constexpr (EXT) pre_l = plo[jn];
    }
    if constexpr (EXT || GATHER) {
      jerk_tile<R, GUARD, EXT>(tile_p[b], tile_v[b], tile_l[b], xi, yi, zi, ui, vi, wi, lxi, lyi, lzi, sa, sj, eps2);
    } else if constexpr (!GUARD) {
      // THE ONE EXCEPTION: the fp32 shared step keeps jerk_tile<R, GUARD, false> written out in
      // the kernel, statement for statement.  Called as a function the same operations came out in another block order
      // and the packed R = 2 loop was scheduled with its velocity reads behind the first v_rsq_f32: at N = 4,096, one
      // wave per SIMD and nothing to hide the LDS latency, the step measured 1.099 x the parent (spread 1.032).
      constexpr int H = R / 2;
      f2 px[H], py[H], pz[H], pu[H], pv[H], pw[H], ax[H], ay[H], az[H], jx[H], jy[H], jz[H];
#pragma unroll
      for (int r = 0; r < H; r++) {
        px[r] = f2{xi[2 * r], xi[2 * r + 1]}; py[r] = f2{yi[2 * r], yi[2 * r + 1]}; pz[r] = f2{zi[2 * r], zi[2 * r + 1]};
        pu[r] = f2{ui[2 * r], ui[2 * r + 1]}; pv[r] = f2{vi[2 * r], vi[2 * r + 1]}; pw[r] = f2{wi[2 * r], wi[2 * r + 1]};
        ax[r] = ay[r] = az[r] = jx[r] = jy[r] = jz[r] = f2{0.f, 0.f};
      }
      constexpr int NS = R >= 4 ? 1 : 2;
#pragma unroll 4
      for (int k = 0; k < TS; k += NS) {
        float4 sp[NS], sv[NS];
#pragma unroll
        for (int q = 0; q < NS; q++) { sp[q] = tile_p[b][k + q]; sv[q] = tile_v[b][k + q]; }
        jerk_pk<R, NS, false>(sp, sv, sp, px, py, pz, pu, pv, pw, px, py, pz, ax, ay, az, jx, jy, jz, eps2);  // (residuals: not read)
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
      for (int k = 0; k < TS; k++)
        jerk_guard<R, false>(tile_p[b][k], tile_v[b][k], tile_p[b][k], xi, yi, zi, ui, vi, wi, xi, yi, zi, ax, ay, az, jx, jy,
                             jz, eps2);  // (residuals: not read)
#pragma unroll
      for (int r = 0; r < R; r++) {
        sa[0][r] += (double)ax[r]; sa[1][r] += (double)ay[r]; sa[2][r] += (double)az[r];
        sj[0][r] += (double)jx[r]; sj[1][r] += (double)jy[r]; sj[2][r] += (double)jz[r];
      }
    }
  }

  float4* oa = pa + (size_t)blockIdx.y * n_pad;
  float4* oj = pj + (size_t)blockIdx.y * n_pad;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int k = tbase + r * kBlock + tid;  // k < n_pad by construction
    oa[k] = make_float4((float)sa[0][r], (float)sa[1][r], (float)sa[2][r], 0.f);
    oj[k] = make_float4((float)sj[0][r], (float)sj[1][r], (float)sj[2][r], 0.f);
  }
}

// ---------------------------------------------------------------------------------
// Finalize: a1 = G sum_splits pa, j1 = G sum_splits pj (fp64, split order), rounded to fp32; then
//   correct = 1   the corrector (hermite_correct<EXT>): v <- v1, x <- x1, acc_old <- a, acc <- a1, jerk <- j1
//   correct = 0   acc4 given: acc4 <- {a1, 0}, acc_* untouched; else acc_* <- a1.  jerk <- {j1, 0}.  Touches no state, so
//                 the fp32 instantiation serves the extended evaluations that do not correct.
// Both forms reduce min |a1| / |j1| over the bodies with |j1| > 0 into the hint word (block_min_ratio).
// ---------------------------------------------------------------------------------
template <bool EXT>
__global__ __launch_bounds__(kBlock) void hermite_finalize_kernel(const float4* __restrict__ pa,
                                                                  const float4* __restrict__ pj, int splits, int n_pad,
                                                                  int n, float G, int correct, float dt, HermiteArrays d,
                                                                  HermiteLo lo, float4* __restrict__ acc4,
                                                                  float4* __restrict__ jerk,
                                                                  unsigned int* __restrict__ hint) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  float ratio = INFINITY;
  if (i < n) {
    float a1[3], j1[3];
    jerk_sum_splits(pa, pj, splits, n_pad, i, G, a1, j1);
    const double a2 = (double)a1[0] * a1[0] + (double)a1[1] * a1[1] + (double)a1[2] * a1[2];
    const double j2 = (double)j1[0] * j1[0] + (double)j1[1] * j1[1] + (double)j1[2] * j1[2];
    if (j2 > 0.0) ratio = (float)sqrt(a2 / j2);
    if (correct) {
      hermite_correct<EXT>((double)dt, d, lo, i, jerk, a1[0], a1[1], a1[2], j1[0], j1[1], j1[2]);
    } else if (acc4) {
      acc4[i] = make_float4(a1[0], a1[1], a1[2], 0.f);
    } else {
      d.ax[i] = a1[0]; d.ay[i] = a1[1]; d.az[i] = a1[2];
    }
    jerk[i] = make_float4(j1[0], j1[1], j1[2], 0.f);
  }
  block_min_ratio(ratio, hint);
}

void hermite_launch_jerk(const nbody_hip_ctx* ctx, const OneSidedShape& s, bool guard, const float4* posm, const float4* vel,
                         const float4* plo, const int* list, int n_targets, int n, float4* pa, float4* pj, float eps2) {
  with_flag(s.R == 4, [&](auto R4) {
    with_flag(guard, [&](auto GD) {
      with_flag(plo != nullptr, [&](auto EX) {
        with_flag(list != nullptr, [&](auto GA) {
          hipLaunchKernelGGL((direct_jerk_kernel<decltype(R4)::value ? 4 : 2, decltype(GD)::value, decltype(EX)::value,
                                                 decltype(GA)::value>),
                             dim3(s.blocks_x, s.splits), dim3(kBlock), 0, ctx->stream, posm, vel, plo, list, n_targets, n,
                             s.src_per_split, pa, pj, s.n_pad, eps2);
        });
      });
    });
  });
}

int hermite_check_arrays(const nbody_hip_ctx* ctx, const nbody_particle_data* d, bool need_old) {
  if (!d) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null particle data");
  if (d->count == 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count must be greater than 0");
  if (d->count > 0x3fffffffu) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "body count exceeds 2^30");
  if (!d->pos_x || !d->pos_y || !d->pos_z || !d->vel_x || !d->vel_y || !d->vel_z || !d->acc_x || !d->acc_y ||
      !d->acc_z || !d->mass)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null arrays");
  if (need_old && (!d->acc_old_x || !d->acc_old_y || !d->acc_old_z))
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null acc_old arrays");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, d->pos_x) != hipSuccess) {
    (void)hipGetLastError();  // memory the runtime does not know: the launch will tell
  } else if (at.type == hipMemoryTypeDevice && at.device != ctx->device) {
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle data lives on device %d, the context on device %d", at.device,
                    ctx->device);
  }
  return NBODY_HIP_OK;
}

// One evaluation at the state (x, v) advanced by the predictor over dt (0: at the state itself), then the finalize
// pass.  Workspaces: ctx->posm holds {xp, m}, {vp, 0} and, in extended state precision, {xp_lo, 0} (2 or 3 n float4; with
// lo4 given the third is the caller's array and the pack is the fp32 one), ctx->partial the split sums of a and j.
int hermite_evaluate(nbody_hip_ctx* ctx, const nbody_particle_data* d, const HermiteLo* lo, const float4* lo4, float G,
                     float eps, float dt, int correct, const float4* jerk_in, float4* acc4, float4* jerk_out,
                     unsigned int* hint) {
  // plan
  const size_t n = d->count;
  const float eps2 = eps * eps;
  const OneSidedShape s = one_sided_shape(no_tuning(), n, n);
  const bool guard = direct_guard(eps2);
  // reserve
  if (int rc = ctx->posm.reserve((lo || lo4 ? 3 : 2) * n * sizeof(float4))) return rc;
  if (int rc = ctx->partial.reserve(2 * s.rows() * sizeof(float4))) return rc;
  float4* posm = static_cast<float4*>(ctx->posm.ptr);
  float4* vel = posm + n;
  float4* plo_own = lo ? vel + n : nullptr;
  float4* pa = static_cast<float4*>(ctx->partial.ptr);
  float4* pj = pa + s.rows();
  // predict and pack, sweep, finalize
  const int blocks = (int)((n + kBlock - 1) / kBlock);
  with_flag(lo != nullptr, [&](auto EX) {
    hipLaunchKernelGGL(hermite_predict_pack_kernel<decltype(EX)::value>, dim3(blocks), dim3(kBlock), 0, ctx->stream,
                       d->pos_x, d->pos_y, d->pos_z, d->vel_x, d->vel_y, d->vel_z, d->acc_x, d->acc_y, d->acc_z, d->mass,
                       lo ? *lo : HermiteLo{}, jerk_in, (int)n, dt, posm, vel, plo_own, hint);
  });
  NBH_LAUNCH_CHECK();
  hermite_launch_jerk(ctx, s, guard, posm, vel, lo4 ? lo4 : plo_own, nullptr, (int)n, (int)n, pa, pj, eps2);
  NBH_LAUNCH_CHECK();
  with_flag(lo && correct, [&](auto EX) {
    hipLaunchKernelGGL(hermite_finalize_kernel<decltype(EX)::value>, dim3(blocks), dim3(kBlock), 0, ctx->stream, pa, pj,
                       s.splits, s.n_pad, (int)n, G, correct, dt, hermite_arrays(d), lo && correct ? *lo : HermiteLo{}, acc4,
                       jerk_out, hint);
  });
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}

// the residuals <- 0, ordered on the context's stream: six planes of max_particles floats (each padded to 256 bytes),
// allocated at first use
int hermite_lo_zero(nbody_hip_ctx* ctx, size_t max_particles, float** mem, HermiteLo* lo) {
  const size_t plane = ((max_particles * sizeof(float) + 255) & ~(size_t)255) / sizeof(float);
  NBH_HIP(hipSetDevice(ctx->device));
  if (!*mem) {
    NBH_HIP(hipMalloc(reinterpret_cast<void**>(mem), 6 * plane * sizeof(float)));
    float* b = *mem;
    *lo = HermiteLo{b, b + plane, b + 2 * plane, b + 3 * plane, b + 4 * plane, b + 5 * plane};
  }
  NBH_HIP(hipMemsetAsync(*mem, 0, 6 * plane * sizeof(float), ctx->stream));
  return NBODY_HIP_OK;
}

// X, V ([n][3], fp64, host) -> hi into the particle data, lo (when the handle is in extended mode) into the residuals
int hermite_state_set_f64(nbody_hip_ctx* ctx, nbody_particle_data* d, const HermiteLo* lo, const double* pos,
                          const double* vel) {
  const size_t n = d->count;
  std::vector<float> buf(12 * n);
  for (size_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) {
      const double x = pos[3 * i + c], v = vel[3 * i + c];
      const float xh = (float)x, vh = (float)v;
      buf[(size_t)c * n + i] = xh;
      buf[(size_t)(3 + c) * n + i] = vh;
      buf[(size_t)(6 + c) * n + i] = (float)(x - (double)xh);
      buf[(size_t)(9 + c) * n + i] = (float)(v - (double)vh);
    }
  float* hi[6] = {d->pos_x, d->pos_y, d->pos_z, d->vel_x, d->vel_y, d->vel_z};
  for (int c = 0; c < 6; c++)
    NBH_HIP(hipMemcpyAsync(hi[c], &buf[(size_t)c * n], n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (lo) {
    float* l[6] = {lo->x, lo->y, lo->z, lo->vx, lo->vy, lo->vz};
    for (int c = 0; c < 6; c++)
      NBH_HIP(hipMemcpyAsync(l[c], &buf[(size_t)(6 + c) * n], n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  NBH_HIP(hipStreamSynchronize(ctx->stream));
  return NBODY_HIP_OK;
}

int hermite_state_get_f64(nbody_hip_ctx* ctx, const nbody_particle_data* d, const HermiteLo* lo, double* pos, double* vel) {
  const size_t n = d->count;
  std::vector<float> buf(12 * n, 0.0f);
  const float* hi[6] = {d->pos_x, d->pos_y, d->pos_z, d->vel_x, d->vel_y, d->vel_z};
  for (int c = 0; c < 6; c++)
    NBH_HIP(hipMemcpyAsync(&buf[(size_t)c * n], hi[c], n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (lo) {
    const float* l[6] = {lo->x, lo->y, lo->z, lo->vx, lo->vy, lo->vz};
    for (int c = 0; c < 6; c++)
      NBH_HIP(hipMemcpyAsync(&buf[(size_t)(6 + c) * n], l[c], n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  NBH_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) {
      pos[3 * i + c] = (double)buf[(size_t)c * n + i] + (double)buf[(size_t)(6 + c) * n + i];
      vel[3 * i + c] = (double)buf[(size_t)(3 + c) * n + i] + (double)buf[(size_t)(9 + c) * n + i];
    }
  return NBODY_HIP_OK;
}

}  // namespace nbh

using namespace nbh;

// (the fields every Hermite handle has, and what the entry points do with them: hermite_handle.h)
struct nbody_hip_hermite : HermiteHandleCore {
  static constexpr const char *kNoun = "Hermite integrator", *kOwner = "integrator's";
  nbody_hip_hermite(nbody_hip_ctx* c, size_t n) : HermiteHandleCore(c, n, kNoun, kOwner) {}
  float4* jerk = nullptr;        // {jx, jy, jz, 0} of the last evaluation, caller order; allocated at first use
  unsigned int* hint = nullptr;  // order-preserving integer of min |a| / |j| of the last evaluation
};

static int hermite_eval(nbody_hip_hermite* h, nbody_particle_data* d, float G, float eps, float dt, int correct) {
  return hermite_evaluate(h->ctx, d, h->lo_or_null(), nullptr, G, eps, dt, correct, correct ? h->jerk : nullptr, nullptr,
                          h->jerk, h->hint);
}

static int hermite_reserve(nbody_hip_hermite* h) {
  if (h->jerk) return NBODY_HIP_OK;
  NBH_HIP(hipMalloc(reinterpret_cast<void**>(&h->jerk), h->max_particles * sizeof(float4) + 256));
  h->hint = reinterpret_cast<unsigned int*>(h->jerk + h->max_particles);
  return NBODY_HIP_OK;
}

static int hermite_prime(nbody_hip_hermite* h, nbody_particle_data* d, float G, float eps) {
  if (int rc = hermite_reserve(h)) return rc;
  h->primed = false;
  if (int rc = hermite_eval(h, d, G, eps, 0.0f, 0)) return rc;
  handle_primed_for(h, d, G, eps);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_create(nbody_hip_ctx* ctx, size_t max_particles, nbody_hip_hermite** out) {
  if (int rc = handle_create_check(ctx, max_particles, out)) return rc;
  *out = new nbody_hip_hermite(ctx, max_particles);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_destroy(nbody_hip_hermite* h) {
  if (!h) return NBODY_HIP_OK;
  NBH_DESTROY_BEGIN
  handle_free(h, h->jerk);
  handle_free(h, h->lo_mem);
  delete h;
  NBH_DESTROY_END
}

extern "C" int nbody_hip_hermite_prime(nbody_hip_hermite* h, nbody_particle_data* d, float G, float eps) {
  if (int rc = handle_check(h, d, "a Hermite priming")) return rc;
  if (int rc = check_eps(eps)) return rc;
  NBH_HIP(hipSetDevice(h->ctx->device));
  return hermite_prime(h, d, G, eps);
}

extern "C" int nbody_hip_hermite_invalidate(nbody_hip_hermite* h) {
  if (int rc = handle_null(h)) return rc;
  return handle_invalidate(h);
}

extern "C" int nbody_hip_hermite_set_precision(nbody_hip_hermite* h, int mode) {
  if (int rc = handle_precision_check(h, mode)) return rc;
  if (mode == h->precision) return NBODY_HIP_OK;
  return handle_precision_switch(h, mode);
}

extern "C" int nbody_hip_hermite_get_precision(nbody_hip_hermite* h, int* mode) {
  return handle_get_precision(h, mode);
}

extern "C" int nbody_hip_hermite_set_state_f64(nbody_hip_hermite* h, nbody_particle_data* d, const double* pos_host,
                                               const double* vel_host) {
  if (int rc = handle_state_check(h, d, pos_host, vel_host, "setting the extended state")) return rc;
  return handle_set_state(h, d, pos_host, vel_host);
}

extern "C" int nbody_hip_hermite_get_state_f64(nbody_hip_hermite* h, nbody_particle_data* d, double* pos_host,
                                               double* vel_host) {
  if (int rc = handle_state_check(h, d, pos_host, vel_host, "reading the extended state")) return rc;
  return handle_get_state(h, d, pos_host, vel_host);
}

extern "C" int nbody_hip_hermite_step(nbody_hip_hermite* h, nbody_particle_data* d, float G, float eps, float dt,
                                      int steps) {
  if (int rc = handle_check(h, d, "a Hermite step")) return rc;
  if (int rc = check_dt(dt)) return rc;
  if (steps < 1) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "steps must be at least 1");
  if (int rc = check_eps(eps)) return rc;
  NBH_HIP(hipSetDevice(h->ctx->device));
  if (!handle_primed_same(h, d, G, eps))
    if (int rc = hermite_prime(h, d, G, eps)) return rc;
  for (int s = 0; s < steps; s++)
    if (int rc = hermite_eval(h, d, G, eps, dt, 1)) {
      h->primed = false;
      return rc;
    }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_jerk(nbody_hip_hermite* h, nbody_float4* out_device) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a jerk read-out");
  if (!out_device) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  if (!h->primed) return handle_not_primed(h);
  NBH_HIP(hipSetDevice(h->ctx->device));
  NBH_HIP(hipMemcpyAsync(out_device, h->jerk, h->count * sizeof(float4), hipMemcpyDeviceToDevice, h->ctx->stream));
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_suggest_dt(nbody_hip_hermite* h, float eta, float* out) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a time-step hint");
  if (!out) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  if (!(eta > 0.0f) || !finite_f(eta)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "eta must be positive and finite");
  if (!h->primed) return handle_not_primed(h);
  NBH_HIP(hipSetDevice(h->ctx->device));
  unsigned int* host = reinterpret_cast<unsigned int*>(h->ctx->host_scalar);
  NBH_HIP(hipMemcpyAsync(host, h->hint, sizeof(unsigned int), hipMemcpyDeviceToHost, h->ctx->stream));
  NBH_HIP(hipStreamSynchronize(h->ctx->stream));
  const unsigned int o = *host;
  const unsigned int u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;  // ordered_to_float on the host
  float r;
  memcpy(&r, &u, sizeof(r));
  *out = eta * r;  // +inf when no body has |j| > 0
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_direct_acc_jerk(nbody_hip_ctx* ctx, nbody_particle_data* d, float G, float eps,
                                         nbody_float4* acc_out, nbody_float4* jerk_out) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  NBH_NOT_CAPTURABLE(ctx, "a force-and-jerk evaluation");
  if (int rc = hermite_check_arrays(ctx, d, false)) return rc;
  if (!jerk_out) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null jerk output");
  if (int rc = check_eps(eps)) return rc;
  NBH_HIP(hipSetDevice(ctx->device));
  if (int rc = ctx->reduce.reserve(256)) return rc;  // the hint word of this evaluation (not kept)
  return hermite_evaluate(ctx, d, nullptr, nullptr, G, eps, 0.0f, 0, nullptr, reinterpret_cast<float4*>(acc_out),
                          reinterpret_cast<float4*>(jerk_out), static_cast<unsigned int*>(ctx->reduce.ptr));
}

extern "C" int nbody_hip_direct_acc_jerk_ext(nbody_hip_ctx* ctx, nbody_particle_data* d, const nbody_float4* pos_lo_device,
                                             float G, float eps, nbody_float4* acc_out, nbody_float4* jerk_out) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  NBH_NOT_CAPTURABLE(ctx, "a force-and-jerk evaluation");
  if (int rc = hermite_check_arrays(ctx, d, false)) return rc;
  if (!pos_lo_device) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null position residuals");
  if (!jerk_out) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null jerk output");
  if (int rc = check_eps(eps)) return rc;
  NBH_HIP(hipSetDevice(ctx->device));
  if (int rc = ctx->reduce.reserve(256)) return rc;  // the hint word of this evaluation (not kept)
  return hermite_evaluate(ctx, d, nullptr, reinterpret_cast<const float4*>(pos_lo_device), G, eps, 0.0f, 0, nullptr,
                          reinterpret_cast<float4*>(acc_out), reinterpret_cast<float4*>(jerk_out),
                          static_cast<unsigned int*>(ctx->reduce.ptr));
}
