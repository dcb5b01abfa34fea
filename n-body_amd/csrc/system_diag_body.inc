// system_diag_body.inc -- the body of system_diag_kernel and system_diag_live_kernel (system_diag.hip), ONE text included
// into both, as hermite_batch_resident_body.inc is: included as text, the existing kernel keeps its instruction stream bit
// for bit (tools/disasm_diff.py).  The including kernel provides the argument A (DiagArgs), the constant LIVE and, when it
// is true, live / live_stride: the live body count of system s is live[s * live_stride] (ensemble MERGERS).
  __shared__ double tile[7][kDiagTile];
  __shared__ double wave_sum[kDiagWaves][kDiagSums];
  __shared__ DiagMin wave_min[kDiagWaves][2];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  nbody_hip_system_diag* const out = A.out + s;

  // the system's range, checked before anything is indexed by it
  unsigned long long o0 = 0ull, o1 = A.single_n;
  if (A.offsets) {
    o0 = A.offsets[s];
    o1 = A.offsets[s + 1];
  }
  o0 = diag_uniform_u64(o0);
  o1 = diag_uniform_u64(o1);
  if (!(o0 < o1 && o1 <= A.count && o1 - o0 <= (unsigned long long)kDiagMaxN)) {  // (uniform)
    if (tid == 0) {
      out->n = 0;
      out->status = 1;
    }
    return;
  }
  const size_t first = (size_t)o0;
  int n_slots = diag_uniform_i((int)(o1 - o0));  // 1 <= n <= 4,096
  if constexpr (LIVE) {
    // the live bodies are the first live[s] slots of the range: only ever fewer than the validated n
    const int nl = diag_uniform_i((int)live[(size_t)s * live_stride]);
    if (nl >= 1 && nl < n_slots) n_slots = nl;
  }
  const int n = n_slots;

  const DiagCells cells = diag_cells(n, kDiagThreads);
  int a, b, r0, r1;
  diag_worker_cells(cells, tid, &a, &b, &r0, &r1);

  DiagSums sums;
  diag_sums_zero(sums);
  DiagMin sep = diag_min_none(INFINITY), bind = diag_min_none(0.0);

  for (int t0 = 0; t0 < n; t0 += kDiagTile) {  // (uniform trip count: the barriers)
    const int t1 = min(t0 + kDiagTile, n);
    if (t0 != 0) __syncthreads();  // the last tile has been read
    for (int k = t0 + tid; k < t1; k += kDiagThreads) {
      const DiagBody q = diag_load(A, first + (size_t)k);
      const int e = k - t0;
      tile[0][e] = q.x; tile[1][e] = q.y; tile[2][e] = q.z;
      tile[3][e] = q.vx; tile[4][e] = q.vy; tile[5][e] = q.vz;
      tile[6][e] = q.m;
      diag_body_add(sums, q);
    }
    __syncthreads();
    for (int r = r0; r < r1; r++) {
      DiagRun run[2];
      diag_row_runs(cells, a, b, r, t0, t1, &run[0], &run[1]);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (run[h].jlo >= run[h].jhi) continue;
        const int i = run[h].i;  // i < n
        const DiagBody ti = diag_load(A, first + (size_t)i);
        for (int j = run[h].jlo; j < run[h].jhi; j++) {  // t0 <= j < t1
          const int e = j - t0;
          const DiagBody sj{tile[0][e], tile[1][e], tile[2][e], tile[3][e], tile[4][e], tile[5][e], tile[6][e]};
          const DiagPair p = diag_pair(ti, sj, A.G, A.eps2);
          sums.v[kDiagSums - 1] += p.term;
          diag_min_take(sep, p.r, i, j);
          if (p.bindable) diag_min_take(bind, p.eb, i, j);
        }
      }
    }
  }

  // the wave: lane l takes lane l + off at off = 32, 16, .., 1; then the four waves in order
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kDiagSums; k++) sums.v[k] += __shfl_down(sums.v[k], off, kWave);
    diag_min_merge(sep, diag_min_shfl_down(sep, off));
    diag_min_merge(bind, diag_min_shfl_down(bind, off));
  }
  if ((tid & (kWave - 1)) == 0) {
    const int w = tid / kWave;
#pragma unroll
    for (int k = 0; k < kDiagSums; k++) wave_sum[w][k] = sums.v[k];
    wave_min[w][0] = sep;
    wave_min[w][1] = bind;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < kDiagWaves; w++) {
#pragma unroll
    for (int k = 0; k < kDiagSums; k++) sums.v[k] += wave_sum[w][k];
    diag_min_merge(sep, wave_min[w][0]);
    diag_min_merge(bind, wave_min[w][1]);
  }
  DiagBody bi{}, bj{};
  if (bind.i >= 0 && bind.v < 0.0) {  // 0 <= bind.i < bind.j < n
    bi = diag_load(A, first + (size_t)bind.i);
    bj = diag_load(A, first + (size_t)bind.j);
  }
  diag_finish(sums, sep, bind, bi, bj, A.G, n, out);
