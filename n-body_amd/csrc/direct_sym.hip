// direct_sym.hip -- Direct N^2 exploiting Newton's third law (action = -reaction), gfx950.
//
// Same sum as direct.hip (and as computeForcesDirectKernel, src/cuda/force_direct.cu:10-85):
//     a_i = G sum_{j != i} m_j (r_j - r_i) (|r_j - r_i|^2 + eps^2)^(-3/2),
// but every UNORDERED pair {i, j} is evaluated once and used twice: the shared factor
// g = (d^2 + eps^2)^(-3/2) costs 3 sub + 3 fma + 1 rsq + 2 mul, then a_i += (g m_j) d and
// a_j -= (g m_i) d are 2 mul + 6 fma: 20 issue slots per unordered pair = 10 per ordered pair,
// against 16 for the one-sided kernel (the rsq alone is 4 slots, measured).
//
// Mapping.  Bodies are cut into superblocks of S = 256 R bodies.  Workgroup (A, split) holds
// superblock A in REGISTERS (each lane R bodies, the "I side") and walks the partner superblocks
// B = A + d (mod NB), d in its share of 0 .. NB/2 (a half ring: every unordered superblock pair
// exactly once; d = 0 is the diagonal, handled without reaction).  A partner is visited in chunks
// of 64 bodies (the "J side"): every wave loads the chunk with lane l holding J body l, together
// with a reaction accumulator that TRAVELS WITH THE BODY.  In each of 64 steps a lane pairs its R
// bodies with the J body it currently holds, adds the reaction into the travelling accumulator,
// and the seven J registers {x, y, z, m, hx, hy, hz} are rotated one lane along the wave
// (v_mov_b32_dpp wave_rol:1).  After 64 steps everything is back in its home lane.  The four
// waves of the block then combine their reactions through LDS (plain stores + barrier) and one
// wave adds the 64 x 3 sums to the global fp64 accumulator with hardware f64 atomics (lossless
// across XCDs, measured ~180 G adds/s).  The I-side sums stay in registers for the whole kernel
// (fp32 per 4 chunks, folded into fp64) and are added once at the end.
//
// With the atomics the result depends on their order in the last bit; the DET form (default for all pairs, see
// below) gives every contribution a slot of its own and is bitwise reproducible like direct.hip; agreement with
// the oracle is the same 1e-5 either way.  Used for the single-GPU all-pairs case (targets == sources) and, as
// RECT, for shard pairs; the one-sided kernel remains the path for N < 12,288 and for eps^2 < 1e-12.

#include <type_traits>

#include "common.h"

namespace nbh {

typedef float f2 __attribute__((ext_vector_type(2)));

// one-lane rotation of a wave64 register: lane l receives the value of lane (l + 1) & 63
__device__ __forceinline__ float wave_rot1(float v) {
  // mov_dpp (no "old" operand): every lane is written, so nothing has to be initialised first
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x134 /* wave_rol:1 */, 0xF, 0xF, false));
}

// R even.  grid = (NB_I, splits), block = 256.
// RECT = false: one body set; partner offsets d in 0 .. NB/2 (half ring), d = 0 without reaction.
// RECT = true : two DISJOINT body sets I (n bodies, posm) and J (nj bodies, posj): every I x J pair
//               once; offsets d = 0 .. NBJ-1 address the J superblocks directly; the reactions go to
//               accj64 (the sharded path sends them back to the owner of the J bodies).
//
// EQM: equal-mass specialisation.  When every body of the call has the same mass m0 > 0 (decided
// on the DEVICE from a min/max reduction, no host round trip: both instantiations are launched
// and the one that does not apply returns at once) the two multiplications g*m_j and g*m_i are
// dropped from every pair (18 instead of 20 issue slots per unordered pair) and m0 is applied once
// to the finished sums.
// (kSymBlocksPerCU workgroups aimed at per CU, at least kSymMinChunks chunks per workgroup: direct_plan.h)
constexpr float kFar = 1.0e18f;  // padding bodies sit here: (3e36)^-3/2 underflows to 0, no mass test needed

// DET: deterministic sums.  Instead of fp64 atomics every contribution gets a slot of its own, written once
// with plain (coalesced) stores; the finalize kernel adds a body's slots in a fixed order.  Bitwise
// reproducible like the reference's one-thread-per-body loop (force_direct.cu:10-85).
//   all pairs : the reaction of the partner at ring offset d -> REACTION slot d - 1 of the receiving body,
//               the I-side sum of split s -> I-SIDE slot s of the body's own superblock;
//   two sets  : the reaction of I superblock A on a J body -> reaction slot A of the J set, the I-side sum
//               of split s -> I-side slot s of the I set.
// A reaction is ONE fp32 number (the sum of the four waves' fp32 sums of a 64-step rotation), so its slot is
// a float: 12 bytes per (body, partner) instead of the 24 of round 2; the I-side sums are fp64.  The equal-
// mass factor m0 is applied by the finalize kernel.  Slot planes: 12 D + 24 splits bytes per body
// (1.9 GB at N = 2^20, 16 bodies per lane: D = 128, 16 splits).
//   acc64  : I-side accumulator -- atomics: [3][plane_i] doubles; DET: [splits][3][plane_i] doubles
//   accj   : reaction accumulator -- atomics: [3][plane] doubles (all pairs: the same array as acc64; two sets:
//            the J set's); DET: [D or NBI][3][plane] FLOATS
//
// RL: accumulator residency.  The fp64 I-side sums of bodies 0 .. RL-1 of a lane live in LDS, those of bodies
// RL .. R-1 in registers.  R = 16 with every sum in LDS (RL = 16) takes 96 KiB + the slab: ONE workgroup per CU, one
// wave per SIMD.  RL = 12 takes 72 KiB + the slab (as R = 12 does) and keeps the last four bodies' sums in 24 VGPRs:
// TWO workgroups per CU, declared with the launch bounds so that the registers are held to 256.  Where a sum lives
// changes no addition and no order of additions: both forms give the same bits.
constexpr int sym_RL(int R) { return sym_residency(R, -1, false, false); }  // (direct_plan.h: who takes which, and why)
template <int R, bool RECT, bool EQM, bool DET = false, int RL = sym_RL(R)>
__global__ __launch_bounds__(kBlock, (R >= 16 && RL < R) ? 2 : 1) void direct_sym_kernel(const float4* __restrict__ posm, int n,
                                                            const float4* __restrict__ posj, int nj,
                                                            int NB, int NBJ, int chunks_per_split,
                                                            double* __restrict__ acc64,
                                                            void* __restrict__ accj,
                                                            size_t plane_i, size_t plane_j,
                                                            const unsigned int* __restrict__ mass_range,
                                                            float eps2) {
  // mass_range = order-preserving encodings {min_I, max_I, min_J, max_J}
  const bool uniform = mass_range[0] == mass_range[1] && mass_range[2] == mass_range[3] &&
                       mass_range[0] == mass_range[2] && ordered_to_float(mass_range[0]) > 0.f;
  if (uniform != EQM) return;  // the other instantiation handles this call
  const float m0 = EQM ? ordered_to_float(mass_range[0]) : 1.0f;
  constexpr int S = kBlock * R;
  __shared__ float slab[2][4][3][64];  // per-wave reaction sums of a chunk, double buffered
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int A = blockIdx.x;
  const int D = RECT ? NBJ - 1 : NB / 2;     // largest partner offset
  // the block's share of the flat list of (partner offset d, 64-body chunk c) pairs: splitting at
  // chunk granularity (not whole partners) gives enough workgroups to fill the last round at
  // mid sizes (65,536 bodies: 64 superblocks x 33 offsets is only two rounds of the chip)
  constexpr int CPB = kBlock * R / 64;
  const int q0 = blockIdx.y * chunks_per_split;
  const int q1 = min((D + 1) * CPB, q0 + chunks_per_split);
  if (q0 >= q1) {
    if constexpr (DET) {  // an empty share still owns an I-side slot: it must read as zero
#pragma unroll
      for (int r = 0; r < R; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
          acc64[((size_t)blockIdx.y * 3 + c) * plane_i + (size_t)(A * S + r * kBlock + tid)] = 0.0;
    }
    return;
  }

  // I side: R bodies per lane, packed in pairs
  f2 xi[R / 2], yi[R / 2], zi[R / 2], mi[R / 2];
#pragma unroll
  for (int r = 0; r < R / 2; r++) {
    float4 p0 = make_float4(kFar, kFar, kFar, 0.f), p1 = p0;
    const int i0 = A * S + (2 * r) * kBlock + tid, i1 = i0 + kBlock;
    if (i0 < n) p0 = posm[i0];
    if (i1 < n) p1 = posm[i1];
    xi[r] = f2{p0.x, p1.x}; yi[r] = f2{p0.y, p1.y}; zi[r] = f2{p0.z, p1.z}; mi[r] = f2{p0.w, p1.w};
  }
  // fp64 sums of the I side.  R = 16 would need 96 VGPRs for them and push the kernel past the 256
  // architectural VGPRs (the rest are AGPRs, reached through copies -- measured: the fastest and
  // the slowest variant, depending on the allocator's mood); they live in LDS there instead,
  // touched once per 4 chunks, [component][r][thread] so that a wave's accesses are contiguous.
  // R = 16 keeps the sums of its last four bodies in registers all the same (RL = 12, see above): the LDS
  // then leaves room for a second workgroup on the CU.
  static_assert(RL >= 0 && RL <= R && RL % 2 == 0, "whole packed pairs on either side");
  static_assert(R < 12 || RL == R || 3 * RL * kBlock * sizeof(double) + sizeof(slab) <= 80 * 1024,
                "two workgroups per CU need <= 80 KiB of LDS each");
  constexpr int RG = R - RL;  // bodies whose sums are registers
  __shared__ double lacc[RL > 0 ? 3 * RL * kBlock : 1];
  double sx[RG > 0 ? RG : 1], sy[RG > 0 ? RG : 1], sz[RG > 0 ? RG : 1];
#pragma unroll
  for (int k = 0; k < 3 * RL; k++) lacc[k * kBlock + tid] = 0.0;  // own slots only: no barrier needed
#pragma unroll
  for (int r = 0; r < RG; r++) sx[r] = sy[r] = sz[r] = 0.0;
  f2 ax[R / 2], ay[R / 2], az[R / 2];
#pragma unroll
  for (int r = 0; r < R / 2; r++) ax[r] = ay[r] = az[r] = f2{0.f, 0.f};
  const f2 e2 = {eps2, eps2};

  // flat list of chunks: (offset d, chunk c of the partner); S/64 = CPB chunks per partner
  // partner d is skipped when the half ring would visit the pair twice (NB even, d = NB/2, upper half)
  auto partner_valid = [&](int d) { return RECT || !((NB % 2 == 0) && d == D && d > 0 && A >= D); };
  const int nchunks = q1 - q0;

  auto load_chunk = [&](int q) -> float4 {  // q-th chunk of this block's list, body `lane`
    const int d = (q0 + q) / CPB, c = (q0 + q) % CPB;
    const int B = RECT ? d : (A + d) % NB;
    const int j = B * S + c * 64 + lane;
    float4 p = make_float4(kFar, kFar, kFar, 0.f);
    if (RECT) { if (j < nj) p = posj[j]; }
    else if (j < n && partner_valid(d)) p = posm[j];
    return p;  // invalid partner / padding: zero mass, far away -> contributes nothing
  };
  auto flush_chunk = [&](int q) {  // one wave: combine the four waves' sums of chunk q, add to global
    const int pd = (q0 + q) / CPB, pc = (q0 + q) % CPB;
    if constexpr (DET) {
      if (RECT || pd > 0) {  // all pairs: slot pd - 1 of the partner's bodies (a partner the half ring skips
        // contributes zero); two sets: slot A of the J bodies.  Wave-uniform slot base, 32-bit element offsets
        // (a slot's three planes stay far below 2^32 floats)
        const size_t plane = RECT ? plane_j : plane_i;
        float* slot = static_cast<float*>(accj) + (size_t)(RECT ? A : pd - 1) * 3 * plane;
        const unsigned int j = (unsigned int)((RECT ? pd : (A + pd) % NB) * S + pc * 64 + lane), pl = (unsigned int)plane;
        const int sb = q & 1;
        const bool keep = partner_valid(pd);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float v = (slab[sb][0][c][lane] + slab[sb][1][c][lane]) + (slab[sb][2][c][lane] + slab[sb][3][c][lane]);
          slot[c * pl + j] = keep ? v : 0.f;
        }
      }
    } else if ((RECT || pd > 0) && partner_valid(pd)) {
      const int j = (RECT ? pd : (A + pd) % NB) * S + pc * 64 + lane;
      const int sb = q & 1;
      double* dst = RECT ? static_cast<double*>(accj) : acc64;
      const size_t plane = RECT ? plane_j : plane_i;
#pragma unroll
      for (int c = 0; c < 3; c++) {  // component planes: 64 lanes x 8 B contiguous per atomic instruction
        const float v = (slab[sb][0][c][lane] + slab[sb][1][c][lane]) + (slab[sb][2][c][lane] + slab[sb][3][c][lane]);
        unsafeAtomicAdd(&dst[c * plane + (size_t)j], (double)v * (double)m0);
      }
    }
  };

  float4 jnext = load_chunk(0);
  for (int q = 0; q < nchunks; q++) {
    const float4 jcur = jnext;
    if (q + 1 < nchunks) jnext = load_chunk(q + 1);  // next chunk in flight under the math
    const int d = (q0 + q) / CPB;
    const bool react = RECT || d > 0;  // the diagonal superblock pair sees every ordered pair already
    if (q > 0) {
      __syncthreads();  // every wave has stored its sums of chunk q-1
      if (w == (q & 3)) flush_chunk(q - 1);
    }
    float jx = jcur.x, jy = jcur.y, jz = jcur.z, jm = jcur.w;
    float hjx = 0.f, hjy = 0.f, hjz = 0.f;
    auto steps = [&](auto react_tag) {
      constexpr bool REACT = decltype(react_tag)::value;
      constexpr int kStepUnroll = R >= 16 ? 1 : 2;  // two steps in flight, registers permitting
      // packed pairs per phase: all R/2 -- but half of them at a time in the equal-mass kernel with two workgroups per
      // CU, whose two loop bodies then fit 256 registers; the partner wave on the SIMD covers the shorter phases
      constexpr int PH = (R >= 16 && RL < R && EQM) ? R / 4 : R / 2;
#pragma unroll kStepUnroll
      for (int k = 0; k < 64; k++) {
        const f2 sxj = {jx, jx}, syj = {jy, jy}, szj = {jz, jz}, smj = {jm, jm};
        // phases over PH packed pairs at a time: the dependent chain of one pair (r2 -> rsq -> g -> sums)
        // is interleaved with the other pairs' instead of being padded with hazard nops
        f2 dx[PH], dy[PH], dz[PH], g[PH];
        auto phase_g = [&](int b) {
#pragma unroll
          for (int r = 0; r < PH; r++) {
            dx[r] = sxj - xi[b + r]; dy[r] = syj - yi[b + r]; dz[r] = szj - zi[b + r];
            g[r] = __builtin_elementwise_fma(dx[r], dx[r], __builtin_elementwise_fma(dy[r], dy[r], __builtin_elementwise_fma(dz[r], dz[r], e2)));
          }
#pragma unroll
          for (int r = 0; r < PH; r++) {
            g[r].x = __builtin_amdgcn_rsqf(g[r].x);
            g[r].y = __builtin_amdgcn_rsqf(g[r].y);
          }
#pragma unroll
          for (int r = 0; r < PH; r++) g[r] = (g[r] * g[r]) * g[r];
        };
        phase_g(0);
        // the travelling reaction sum rides in the low half of the packed accumulator
        f2 hx = {hjx, 0.f}, hy = {hjy, 0.f}, hz = {hjz, 0.f};
        auto phase_sums = [&](int b) {
#pragma unroll
          for (int r = 0; r < PH; r++) {
            const f2 fj = EQM ? g[r] : g[r] * smj;    // on the I bodies, from J
            ax[b + r] = __builtin_elementwise_fma(fj, dx[r], ax[b + r]);
            ay[b + r] = __builtin_elementwise_fma(fj, dy[r], ay[b + r]);
            az[b + r] = __builtin_elementwise_fma(fj, dz[r], az[b + r]);
            if (REACT) {
              const f2 fi = EQM ? g[r] : g[r] * mi[b + r];  // on the J body, from the I bodies
              hx = __builtin_elementwise_fma(-fi, dx[r], hx);  // a_j -= g m_i d  (neg is an operand modifier)
              hy = __builtin_elementwise_fma(-fi, dy[r], hy);
              hz = __builtin_elementwise_fma(-fi, dz[r], hz);
            }
          }
        };
        phase_sums(0);
        if constexpr (PH < R / 2) {  // the second half of the pairs, in the same registers
          phase_g(PH);
          phase_sums(PH);
        }
        if (REACT) {
          hjx = wave_rot1(hx.x + hx.y); hjy = wave_rot1(hy.x + hy.y); hjz = wave_rot1(hz.x + hz.y);
        }
        jx = wave_rot1(jx); jy = wave_rot1(jy); jz = wave_rot1(jz); jm = wave_rot1(jm);
      }
    };
    if constexpr (R >= 12 && !EQM) {
      // GENERAL masses at 12 / 16 bodies per lane: ONE loop body -- the diagonal superblock pair (d = 0: one partner
      // in D + 1, i.e. 0.8 % of the chunks at N = 2^20) computes its reactions too and drops them at the flush.  Two
      // instantiations of the 64-step loop cost registers: the slot kernel at R = 16 needed 256 VGPRs + 29 AGPR
      // copies (190 ms at N = 2^20, which is why round 2 ran it at R = 12); with one body it fits 246 (171.5 ms).
      // The equal-mass kernel keeps both bodies: with one it needs fewer registers (226) but the schedule the
      // compiler then picks is slower (R = 16: 170 ms against 158, measured, tools/direct_det_probe.py).  Under two
      // workgroups per CU (RL = 12) the one-body form no longer loses to the parent (153.7 ms against 158.1) but
      // still loses to both bodies phased over 4 pairs (PH above: 152.4 ms; DESIGN.md 4.1, same box, alternated).
      (void)react;
      steps(std::true_type{});
    } else {
      if (react) steps(std::true_type{}); else steps(std::false_type{});
    }
    // after 64 one-lane rotations every J body (and its reaction sum) is back in its home lane
    slab[q & 1][w][0][lane] = hjx; slab[q & 1][w][1][lane] = hjy; slab[q & 1][w][2][lane] = hjz;
    if ((q & 3) == 3 || q == nchunks - 1) {  // fold the fp32 sums of <= 256 sources into fp64
#pragma unroll
      for (int r = 0; r < R / 2; r++) {
        if (2 * r < RL) {  // (folds once the loop is unrolled)
          lacc[(0 * RL + 2 * r) * kBlock + tid] += (double)ax[r].x; lacc[(0 * RL + 2 * r + 1) * kBlock + tid] += (double)ax[r].y;
          lacc[(1 * RL + 2 * r) * kBlock + tid] += (double)ay[r].x; lacc[(1 * RL + 2 * r + 1) * kBlock + tid] += (double)ay[r].y;
          lacc[(2 * RL + 2 * r) * kBlock + tid] += (double)az[r].x; lacc[(2 * RL + 2 * r + 1) * kBlock + tid] += (double)az[r].y;
        } else {
          sx[2 * r - RL] += (double)ax[r].x; sx[2 * r + 1 - RL] += (double)ax[r].y;
          sy[2 * r - RL] += (double)ay[r].x; sy[2 * r + 1 - RL] += (double)ay[r].y;
          sz[2 * r - RL] += (double)az[r].x; sz[2 * r + 1 - RL] += (double)az[r].y;
        }
        ax[r] = ay[r] = az[r] = f2{0.f, 0.f};
      }
    }
  }
  __syncthreads();
  if (w == (nchunks & 3)) flush_chunk(nchunks - 1);
  // I side
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int i = A * S + r * kBlock + tid;  // < NB * S: the accumulator is padded to that
    const double fx = r < RL ? lacc[(0 * RL + r) * kBlock + tid] : sx[r < RL ? 0 : r - RL];
    const double fy = r < RL ? lacc[(1 * RL + r) * kBlock + tid] : sy[r < RL ? 0 : r - RL];
    const double fz = r < RL ? lacc[(2 * RL + r) * kBlock + tid] : sz[r < RL ? 0 : r - RL];
    if constexpr (DET) {  // (m0 is applied by the finalize kernel)
      double* slot = acc64 + (size_t)blockIdx.y * 3 * plane_i;
      const unsigned int iu = (unsigned int)i, pl = (unsigned int)plane_i;
      slot[iu] = fx;
      slot[pl + iu] = fy;
      slot[2u * pl + iu] = fz;
    } else {
      unsafeAtomicAdd(&acc64[(size_t)i], fx * (double)m0);
      unsafeAtomicAdd(&acc64[plane_i + (size_t)i], fy * (double)m0);
      unsafeAtomicAdd(&acc64[2 * plane_i + (size_t)i], fz * (double)m0);
    }
  }
}

__global__ void mass_range_init_kernel(unsigned int* enc) {
  if (threadIdx.x < 4) enc[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xffffffffu;  // {min, max, min, max}
}

// min / max of the masses of a packed body set -> enc[0], enc[1] (order-preserving integers)
__global__ __launch_bounds__(kBlock) void mass_range_kernel(const float4* __restrict__ posm, int n,
                                                            unsigned int* __restrict__ enc) {
  __shared__ float red[4][2];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const float m = posm[i].w;
    lo = fminf(lo, m); hi = fmaxf(hi, m);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, 64));
    hi = fmaxf(hi, __shfl_down(hi, off, 64));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w][0] = lo; red[w][1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; k++) { lo = fminf(lo, red[k][0]); hi = fmaxf(hi, red[k][1]); }
    atomicMin(&enc[0], float_to_ordered(fminf(lo, red[0][0])));
    atomicMax(&enc[1], float_to_ordered(fmaxf(hi, red[0][1])));
  }
}

// Where a body's contributions lie: n_i I-side slots (fp64, [slot][3][plane]) and n_r reaction slots (fp32, same
// shape).  Atomic mode: one fp64 slot that already holds everything (n_i = 1, n_r = 0).
struct SlotLayout {
  const double* isl;
  const float* rsl;
  size_t plane;
  int n_i, n_r;
};

// acc = G * (sum of the body's slots, in a fixed order) ; SoA or float4 output ; optional fused Velocity-Verlet kick
// apply_m0: deterministic mode -- the equal-mass kernel stores its sums without the common mass factor
__global__ __launch_bounds__(kBlock) void direct_sym_finalize_kernel(
    SlotLayout eq, SlotLayout gen, int apply_m0, const unsigned int* __restrict__ mass_range, int n, float G,
    float4* __restrict__ acc4, int accumulate, float* __restrict__ ax, float* __restrict__ ay, float* __restrict__ az,
    float* __restrict__ vx, float* __restrict__ vy, float* __restrict__ vz, const float* __restrict__ aox,
    const float* __restrict__ aoy, const float* __restrict__ aoz, float half_dt) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  SlotLayout L = eq;
  double m0 = 1.0;
  if (mass_range) {  // the general-mass instantiation ran with a layout of its own (other bodies per lane)
    const bool uniform = mass_range[0] == mass_range[1] && mass_range[2] == mass_range[3] &&
                         mass_range[0] == mass_range[2] && ordered_to_float(mass_range[0]) > 0.f;
    if (!uniform) L = gen;
    else if (apply_m0) m0 = (double)ordered_to_float(mass_range[0]);
  }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int k = 0; k < L.n_r; k++) {
    const float* p = L.rsl + (size_t)k * 3 * L.plane;
    sx += (double)p[i]; sy += (double)p[L.plane + i]; sz += (double)p[2 * L.plane + i];
  }
  for (int k = 0; k < L.n_i; k++) {
    const double* p = L.isl + (size_t)k * 3 * L.plane;
    sx += p[i]; sy += p[L.plane + i]; sz += p[2 * L.plane + i];
  }
  const double gm = (double)G * m0;
  const float fx = (float)(gm * sx), fy = (float)(gm * sy), fz = (float)(gm * sz);
  if (acc4) {
    float4 o = make_float4(fx, fy, fz, 0.f);
    if (accumulate) { const float4 c = acc4[i]; o.x += c.x; o.y += c.y; o.z += c.z; }
    acc4[i] = o;
  } else {
    ax[i] = fx; ay[i] = fy; az[i] = fz;
    if (vx) {
      vx[i] = kick1(vx[i], aox[i], fx, half_dt);
      vy[i] = kick1(vy[i], aoy[i], fy, half_dt);
      vz[i] = kick1(vz[i], aoz[i], fz, half_dt);
    }
  }
}

static void launch_mass_range(nbody_hip_ctx* ctx, const float4* pi, int ni, const float4* pj, int nj,
                              unsigned int* enc) {
  hipLaunchKernelGGL(mass_range_init_kernel, dim3(1), dim3(64), 0, ctx->stream, enc);
  const int bi = (ni + kBlock - 1) / kBlock, bj = (nj + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(mass_range_kernel, dim3(bi < 256 ? bi : 256), dim3(kBlock), 0, ctx->stream, pi, ni, enc);
  hipLaunchKernelGGL(mass_range_kernel, dim3(bj < 256 ? bj : 256), dim3(kBlock), 0, ctx->stream, pj, nj, enc + 2);
}

// One mass instantiation of direct_sym_kernel at R bodies per lane (one of Rs) with the residency of the call
// (sym_residency, direct_plan.h: at 16 bodies per lane 12 or 16, the deterministic two-set form 16 alone; else the one
// value R has).  A call queues both instantiations; the one whose assumption about the masses fails exits at once
// (decided on the device).
template <bool RECT, bool EQM, bool DET, int... Rs>
static void launch_sym(nbody_hip_ctx* ctx, int R, dim3 grid, const float4* pi, int ni, const float4* pj, int nj, int NB,
                       int NBJ, int per, double* acci, void* accj, const unsigned int* enc, float eps2) {
  with_int<Rs...>(R, [&](auto RC) {
    constexpr int R_ = decltype(RC)::value;
    auto launch = [&](auto RL) {
      hipLaunchKernelGGL((direct_sym_kernel<R_, RECT, EQM, DET, decltype(RL)::value>), grid, dim3(kBlock), 0, ctx->stream,
                         pi, ni, pj, nj, NB, NBJ, per, acci, accj, (size_t)NB * kBlock * R_, (size_t)NBJ * kBlock * R_, enc,
                         eps2);
    };
    if constexpr (R_ == 16 && !(RECT && DET)) with_int<12, 16>(sym_residency(R_, ctx->tune.variant, RECT, DET), launch);
    else launch(std::integral_constant<int, sym_residency(R_, -1, RECT, DET)>{});
  });
}

// free bytes of the current device for the budget rule (slot_budget_allows, direct_plan.h)
static size_t device_free_bytes() {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return kFreeUnknown;
  }
  return free_b;
}
// plan(free_bytes) with the device asked only when the budget rule gets as far as the free memory
template <class Plan>
static auto plan_on_device(bool query_device, Plan&& plan) {
  auto p = plan(kFreeUnknown);
  if (query_device && p.asked_free) p = plan(device_free_bytes());
  return p;
}
DirectPlan device_direct_plan(const nbody_hip_ctx* ctx, size_t n, float eps2, bool query_device) {
  return plan_on_device(query_device, [&](size_t free_bytes) {
    return direct_plan(ctx->tune, n, eps2, ctx->partial.bytes, free_bytes);
  });
}

// All pairs of one set, as planned: reserve, both instantiations, finalize.  Each instantiation (equal masses / general
// masses) has a launch shape of its own.  Deterministic mode: one slot per contribution; every slot is written exactly
// once by the kernel, so nothing has to be cleared.  Taken when asked for (nbody_hip_direct_deterministic) and the slot
// planes fit the budget; "required" (mode 2) turns a miss into an error instead of the atomic form.
int direct_symmetric(nbody_hip_ctx* ctx, DirectPlan plan, const float4* posm, size_t n, float G, float eps2,
                     float4* acc4, int accumulate, float* ax, float* ay, float* az, float* vx,
                     float* vy, float* vz, const float* aox, const float* aoy, const float* aoz,
                     float half_dt) {
  if (plan.required && !plan.det)
    return NBH_FAIL(NBODY_HIP_ERR_RESOURCE, "deterministic Direct sums were required but their slot planes (%zu bytes "
                    "for %zu bodies) exceed the budget (%zu bytes and a quarter of the free device memory)",
                    plan.det_bytes_wanted, n, ctx->tune.det_budget);
  // reserve.  A workspace left over from a much larger problem is given back first (the slot planes are the one big
  // allocation of this library)
  if (ctx->partial.bytes > kLargeWorkspace && ctx->partial.bytes / 4 > plan.bytes && !ctx->capturing) {
    NBH_HIP(hipDeviceSynchronize());
    ctx->partial.release();
  }
  int rc = ctx->partial.reserve(plan.bytes);
  if (rc != NBODY_HIP_OK && plan.det && !plan.required) {
    (void)hipGetLastError();
    plan.demote_to_atomics();
    rc = ctx->partial.reserve(plan.bytes);
  }
  if (rc != NBODY_HIP_OK) return rc;
  const SymShape &eq = plan.eq, &gen = plan.gen;
  char* base = static_cast<char*>(ctx->partial.ptr);
  if (!plan.det) NBH_HIP(hipMemsetAsync(base, 0, plan.bytes, ctx->stream));
  if (int rc2 = ctx->reduce.reserve(64)) return rc2;
  unsigned int* enc = static_cast<unsigned int*>(ctx->reduce.ptr);
  // launches
  const int ni = (int)n;
  launch_mass_range(ctx, posm, ni, posm, ni, enc);
  SlotLayout Leq, Lgen;
  if (plan.det) {
    // [reaction slots: D x 3 float planes][I-side slots: splits x 3 double planes], one layout per instantiation
    // (only one of the two runs; they share the workspace)
    Leq = SlotLayout{reinterpret_cast<const double*>(base + eq.reaction_bytes()), reinterpret_cast<const float*>(base),
                     eq.plane, eq.splits, eq.D};
    Lgen = SlotLayout{reinterpret_cast<const double*>(base + gen.reaction_bytes()), reinterpret_cast<const float*>(base),
                      gen.plane, gen.splits, gen.D};
  } else {
    Leq = Lgen = SlotLayout{reinterpret_cast<const double*>(base), nullptr, eq.plane, 1, 0};
  }
  with_flag(plan.det, [&](auto DET) {
    constexpr bool det = decltype(DET)::value;
    launch_sym<false, true, det, 2, 4, 6, 8, 12, 16>(ctx, eq.R, dim3(eq.NB, eq.splits), posm, ni, posm, ni, eq.NB, eq.NB, eq.per,
                                                     const_cast<double*>(Leq.isl), base, enc, eps2);
    launch_sym<false, false, det, 2, 4, 6, 8, 12, 16>(ctx, gen.R, dim3(gen.NB, gen.splits), posm, ni, posm, ni, gen.NB, gen.NB,
                                                      gen.per, const_cast<double*>(Lgen.isl), base, enc, eps2);
  });
  NBH_LAUNCH_CHECK();
  ctx->last_direct_kernel = plan.kernel();
  // finalize
  const int fblocks = (int)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(direct_sym_finalize_kernel, dim3(fblocks), dim3(kBlock), 0, ctx->stream, Leq, Lgen, plan.det ? 1 : 0, enc,
                     ni, G, acc4, accumulate, ax, ay, az, vx, vy, vz, aox, aoy, aoz, half_dt);
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}

// Two disjoint sets: acc_i (+)= forces on I from J ; acc_j = forces on J from I (the reactions).
// Deterministic form (same switch as the all-pairs kernel): `splits` fp64 I-side slots per I body, NBI fp32
// reaction slots per J body -- a sharded run is then reproducible launch after launch too.
int direct_symmetric_pair(nbody_hip_ctx* ctx, const float4* pi, size_t ni, const float4* pj, size_t nj,
                          float G, float eps2, float4* acc_i, int accumulate_i, float4* acc_j,
                          int accumulate_j) {
  // plan
  PairPlan plan = plan_on_device(true, [&](size_t free_bytes) {
    return pair_plan(ctx->tune, ni, nj, ctx->partial.bytes, free_bytes);
  });
  if (plan.required && !plan.det)
    return NBH_FAIL(NBODY_HIP_ERR_RESOURCE, "deterministic Direct sums were required but their slot planes (%zu bytes) "
                    "exceed the budget", plan.det_bytes_wanted);
  // reserve
  int rc = ctx->partial.reserve(plan.s.bytes());
  if (rc != NBODY_HIP_OK && plan.det && !plan.required) {
    (void)hipGetLastError();
    plan.demote_to_atomics();
    rc = ctx->partial.reserve(plan.s.bytes());
  }
  if (rc != NBODY_HIP_OK) return rc;
  const PairShape& s = plan.s;
  char* base = static_cast<char*>(ctx->partial.ptr);
  double* acci = reinterpret_cast<double*>(base);
  void* accj = base + s.i_bytes();
  if (!s.det) NBH_HIP(hipMemsetAsync(base, 0, s.bytes(), ctx->stream));
  if (int rc2 = ctx->reduce.reserve(64)) return rc2;
  unsigned int* enc = static_cast<unsigned int*>(ctx->reduce.ptr);
  // launches
  launch_mass_range(ctx, pi, (int)ni, pj, (int)nj, enc);
  with_flag(s.det, [&](auto DET) {
    constexpr bool det = decltype(DET)::value;
    launch_sym<true, true, det, 2, 4, 6, 8, 16>(ctx, s.R, dim3(s.NBI, s.splits), pi, (int)ni, pj, (int)nj, s.NBI, s.NBJ, s.per,
                                                acci, accj, enc, eps2);
    launch_sym<true, false, det, 2, 4, 6, 8, 16>(ctx, s.R, dim3(s.NBI, s.splits), pi, (int)ni, pj, (int)nj, s.NBI, s.NBJ, s.per,
                                                 acci, accj, enc, eps2);
  });
  NBH_LAUNCH_CHECK();
  ctx->last_direct_kernel = s.det ? 2 : 1;
  // finalize
  SlotLayout Li, Lj;
  if (s.det) {
    Li = SlotLayout{acci, nullptr, s.plane_i, s.splits, 0};
    Lj = SlotLayout{nullptr, static_cast<const float*>(accj), s.plane_j, 0, s.NBI};
  } else {
    Li = SlotLayout{acci, nullptr, s.plane_i, 1, 0};
    Lj = SlotLayout{static_cast<const double*>(accj), nullptr, s.plane_j, 1, 0};
  }
  // (mass_range is read for the equal-mass factor only in the deterministic form; the atomic form applied it)
  hipLaunchKernelGGL(direct_sym_finalize_kernel, dim3((unsigned)((ni + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     ctx->stream, Li, Li, s.det ? 1 : 0, s.det ? enc : nullptr, (int)ni, G, acc_i, accumulate_i, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f);
  hipLaunchKernelGGL(direct_sym_finalize_kernel, dim3((unsigned)((nj + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     ctx->stream, Lj, Lj, s.det ? 1 : 0, s.det ? enc : nullptr, (int)nj, G, acc_j, accumulate_j, nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f);
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}

}  // namespace nbh
