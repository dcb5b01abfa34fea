// hermite_batch_prime_sweep.inc -- the body of the priming's sweep kernels (hermite_batch.hip), ONE text included into
// both: batch_prime_sweep_kernel (every item of the layout) and batch_reprime_sweep_kernel (the items of the marked systems
// that exist at the LIVE count, behind its two uniform exits; DESIGN.md section 4.21).  The tile body of
// direct_jerk_kernel<2, GUARD, EXT, false> (jerk_tile, hermite_common.h) for one (system, 512-target block, 256-source
// tile), with targets, sources and padding confined to the system.
// It is text and not a function for the reason hermite_batch_resident_body.inc gives: as a __forceinline__ device
// function the same statements kept lines, VGPRs and occupancy but renumbered the registers and changed the SGPR counts of
// all eight sweep kernels; included as text, both kernels keep their instruction streams bit for bit
// (tools/disasm_diff.py).  The including kernel provides: the template flags GUARD and EXT; its arguments posm_all,
// vel_all, plo_all, pa_all, pj_all and eps2; tblock and tile (int, wave-uniform: the work item) and w (BatchSystem: the
// words of the item's system).  The text declares R, the three LDS tiles, tid, first, n, row_off, posm, vel, plo, n_pad and
// tbase itself -- the including kernel must not -- and does not return.
  constexpr int R = kPrimeR;
  __shared__ float4 tile_p[TS];
  __shared__ float4 tile_v[TS];
  __shared__ float4 tile_l[EXT ? TS : 1];
  const int tid = threadIdx.x;
  const int first = uniform_i(w.first), n = uniform_i(w.n);
  const size_t row_off = uniform_u64(w.prime_row_off);
  const float4* posm = posm_all + first;
  const float4* vel = vel_all + first;
  const float4* plo = plo_all + first;  // (extended only)
  const int n_pad = (n + kPrimeTargets - 1) / kPrimeTargets * kPrimeTargets;
  const int tbase = tblock * kPrimeTargets;

  float xi[R], yi[R], zi[R], ui[R], vi[R], wi[R], lxi[R], lyi[R], lzi[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int k = tbase + r * kBlock + tid;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p, l = p;
    if (k < n) {
      p = posm[k];
      v = vel[k];
      if constexpr (EXT) l = plo[k];
    }
    xi[r] = p.x; yi[r] = p.y; zi[r] = p.z;
    ui[r] = v.x; vi[r] = v.y; wi[r] = v.z;
    lxi[r] = l.x; lyi[r] = l.y; lzi[r] = l.z;
  }
  // the tile's sources; padded source: m = 0, at rest at the origin, residual 0
  {
    const int j = tile * TS + tid;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p, l = p;
    if (j < n) {
      p = posm[j];
      v = vel[j];
      if constexpr (EXT) l = plo[j];
    }
    tile_p[tid] = p;
    tile_v[tid] = v;
    if constexpr (EXT) tile_l[tid] = l;
  }
  __syncthreads();

  double sa[3][R], sj[3][R];
#pragma unroll
  for (int r = 0; r < R; r++) sa[0][r] = sa[1][r] = sa[2][r] = sj[0][r] = sj[1][r] = sj[2][r] = 0.0;
  jerk_tile<R, GUARD, EXT>(tile_p, tile_v, tile_l, xi, yi, zi, ui, vi, wi, lxi, lyi, lzi, sa, sj, eps2);

  float4* oa = pa_all + row_off + (size_t)tile * n_pad;
  float4* oj = pj_all + row_off + (size_t)tile * n_pad;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int k = tbase + r * kBlock + tid;  // k < n_pad: tbase is a multiple of 512 below n_pad
    oa[k] = make_float4((float)sa[0][r], (float)sa[1][r], (float)sa[2][r], 0.f);
    oj[k] = make_float4((float)sj[0][r], (float)sj[1][r], (float)sj[2][r], 0.f);
  }
