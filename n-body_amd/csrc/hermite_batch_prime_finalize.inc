// hermite_batch_prime_finalize.inc -- what the priming's finalize does for ONE body (hermite_batch.hip), ONE text included
// into both finalize kernels: batch_prime_finalize_kernel (one thread per body of the ensemble) and
// batch_reprime_finalize_kernel (one workgroup per marked system, a loop over its live bodies; DESIGN.md section 4.21).  The
// sums of hermite_finalize_kernel (rows in tile order in fp64, G in fp64, rounded to fp32) -> acc_*, jerk; then
// block_prime_kernel's rule with the system's dt_max.
// It is text and not a function for the reason hermite_batch_resident_body.inc gives: included as text, both kernels keep
// their instruction streams bit for bit (tools/disasm_diff.py).  The including kernel provides: its arguments G, eta_s, L,
// ax, ay, az, jerk, level, tick and want; i (the body's index in the ensemble) and k (its index in the system); tiles and
// n_pad of the system; pa and pj (the system's rows); and dt (the system's dt_max: in the kernel with one thread per body a
// REFERENCE to dt_max[s], because a copy hoists the load and changes that kernel's stream).
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < tiles; q++) {
    const float4 p = pa[(size_t)q * n_pad + k], r = pj[(size_t)q * n_pad + k];
    sum[0] += (double)p.x; sum[1] += (double)p.y; sum[2] += (double)p.z;
    sum[3] += (double)r.x; sum[4] += (double)r.y; sum[5] += (double)r.z;
  }
  const float a1x = (float)((double)G * sum[0]), a1y = (float)((double)G * sum[1]), a1z = (float)((double)G * sum[2]);
  const float4 j1 = make_float4((float)((double)G * sum[3]), (float)((double)G * sum[4]), (float)((double)G * sum[5]), 0.f);
  ax[i] = a1x; ay[i] = a1y; az[i] = a1z;
  jerk[i] = j1;
  float wnt;
  level[i] = block_prime_level(a1x, a1y, a1z, j1, eta_s, dt, L, &wnt);
  tick[i] = 0u;
  want[i] = wnt;
