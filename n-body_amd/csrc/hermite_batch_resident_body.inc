// hermite_batch_resident_body.inc -- the body of the ensemble's resident kernels (hermite_batch.hip), ONE text included
// into each of them: batch_resident_kernel (plain and event forms), batch_outcomes_kernel (DESIGN.md section 4.19) and
// batch_hierarchy_kernel (section 4.20).
// A kernel cannot call a kernel, and a body shared as an inlined function is optimised once on its own before it is
// inlined, which changed the register allocation of the event forms; included as text, the existing instantiations keep
// their instruction streams bit for bit (tools/disasm_diff.py).  The including kernel provides: the template flags EXT,
// GUARD, the constants EVENTS (records and stop words), TRACK (the pair keys, the radii and the budget: events are
// configured), OUTCOMES (the escape test) and HIERARCHY (the decomposition), and the arguments A, E, O, H and macro_steps.
  const int sidx = blockIdx.x;
  // (the system's words are alike in every thread: scalar registers, so every offset below stays wave-uniform)
  const BatchSystem w = A.sys[sidx];
  const int first = uniform_i(w.first);
  const size_t row_off = uniform_u64(w.row_off);
  const unsigned int status_in = (unsigned int)uniform_i((int)A.status[sidx]);
  // EVENTS: the system's record and budget
  unsigned int stopped_in = 0u, stopped = 0u, ctick = 0u, ttick = 0u;
  unsigned long long limit = 0ull, base = 0ull, ckey = kKeyNone, cmacro = 0ull, tkey = kKeyNone, tmacro = 0ull;
  // OUTCOMES: the system's escape radius and whether its first escape is on record (uniform)
  float r_esc = 0.f;
  bool escaped = false;
  if constexpr (EVENTS) {
    const nbody_hip_batch_event_t ev = E.events[sidx];
    stopped_in = (unsigned int)uniform_i((int)ev.stopped);
    if constexpr (TRACK) limit = uniform_u64(E.limits[sidx]);  // (no events configured: no radii, no budget)
    base = uniform_u64(A.state[sidx].macro_steps);  // macro steps completed before this launch
    ckey = uniform_u64(event_key(ev.closest_d2, ev.closest_i, ev.closest_j));
    cmacro = uniform_u64(ev.closest_macro);
    ctick = (unsigned int)uniform_i((int)ev.closest_tick);
    tkey = uniform_u64(event_key(ev.contact_d2, ev.contact_i, ev.contact_j));
    tmacro = uniform_u64(ev.contact_macro);
    ttick = (unsigned int)uniform_i((int)ev.contact_tick);
  }
  // HIERARCHY: the system's separation radius and whether it is on record as resolved (uniform)
  float r_sep = 0.f;
  bool resolved = false;
  bool outcomes_on = true;
  if constexpr (HIERARCHY) outcomes_on = O.r_esc != nullptr;  // (the hierarchy form alone: no escape radii, no test)
  if constexpr (OUTCOMES) {
    if (outcomes_on) {
      r_esc = __int_as_float(uniform_i(__float_as_int(O.r_esc[sidx])));
      escaped = uniform_i((int)O.out[sidx].escaped) != 0;
    }
  }
  if constexpr (HIERARCHY) {
    r_sep = __int_as_float(uniform_i(__float_as_int(H.r_sep[sidx])));
    resolved = uniform_i((int)H.rec[sidx].resolved) != 0;
  }
  __syncthreads();  // (thread 0 writes the status word and the record at the end)
  if (status_in != 0u || stopped_in != 0u) return;  // given up on, or stopped: nothing of the system is touched

  const ResidentArrays& P = A.p;
  ResidentSystem S;
  S.p.d = HermiteArrays{P.d.x + first,  P.d.y + first,  P.d.z + first,  P.d.vx + first,  P.d.vy + first,  P.d.vz + first,
                        P.d.ax + first, P.d.ay + first, P.d.az + first, P.d.aox + first, P.d.aoy + first, P.d.aoz + first};
  S.p.lo = HermiteLo{};
  if constexpr (EXT)
    S.p.lo = HermiteLo{P.lo.x + first, P.lo.y + first, P.lo.z + first, P.lo.vx + first, P.lo.vy + first, P.lo.vz + first};
  S.p.mass = P.mass + first;
  S.p.jerk = P.jerk + first;
  S.p.level = P.level + first;
  S.p.tick = P.tick + first;
  S.p.want = P.want + first;
  S.p.posm = P.posm + first;
  S.p.vel = P.vel + first;
  S.p.plo = P.plo + first;  // (extended only)
  S.p.pa = P.pa + row_off;
  S.p.pj = P.pj + row_off;
  S.counters = A.counters + (size_t)sidx * kCounters;
  S.radii = nullptr;
  if constexpr (TRACK) S.radii = E.radii + first;
  S.n = uniform_i(w.n);
  S.L = A.L;
  S.G = A.G;
  S.eps2 = A.eps2;
  S.dt_max = __int_as_float(uniform_i(__float_as_int(A.dt_max[sidx])));
  S.eta = A.eta;
  const unsigned int end = 1u << A.L;

  unsigned int status = 0u, last_n = 0u, cur = 0u;
  unsigned long long steps = 0ull, bodies = 0ull, macros = 0ull;
  // EVENTS: the stop conditions (uniform), looked at at a macro boundary: the macro step a contact fell into is completed
  const auto stop_word = [&]() -> unsigned int {
    if ((E.flags & NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT) != 0u && tkey != kKeyNone) return 1u;
    if constexpr (OUTCOMES) {
      if ((O.flags & NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE) != 0u && escaped) return 3u;  // (above the budget)
    }
    if constexpr (HIERARCHY) {
      if ((H.flags & NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED) != 0u && resolved) return 4u;  // (below the escape)
    }
    return limit != 0ull && base + macros >= limit ? 2u : 0u;
  };
  for (int ms = 0; ms < macro_steps && status == 0u; ms++) {
    if constexpr (EVENTS) {
      stopped = stop_word();
      if (stopped != 0u) break;
    }
    bool boundary = false;
    cur = 0u;  // (every advance starts and ends at a boundary: the ticks are re-based in memory)
    for (unsigned int it = 0; it < end + 1u; it++) {
      ResidentStep st;
      if (!resident_block_step<EXT, GUARD, TRACK>(S, cur, st)) {  // (uniform)
        status = 1u;
        break;
      }
      if constexpr (TRACK) {
        if ((E.flags & NBODY_HIP_BATCH_EVENTS_TRACK_CLOSEST) != 0u && st.closest < ckey) {
          ckey = st.closest;  // (strictly less: the earliest block step keeps a tie)
          cmacro = base + macros;
          ctick = st.t;
        }
        if (tkey == kKeyNone && st.contact != kKeyNone) {  // (the first block step with a contact, once)
          tkey = st.contact;
          tmacro = base + macros;
          ttick = st.t;
        }
      }
      steps++;
      bodies += st.n_active;
      last_n = st.n_active;
      if (st.t == end) {
        cur = 0u;
        boundary = true;
        break;
      }
      cur = st.t;
    }
    if (status == 0u && !boundary) status = 2u;  // 2^L + 1 block steps and no boundary
    if (boundary) macros++;
    if constexpr (OUTCOMES) {
      // the escape test at the boundary just counted (uniform condition: the test has barriers), until the first escape
      if (boundary && !escaped && r_esc > 0.f && S.n > 1)
        escaped = batch_outcome_test<EXT>(S, (double)r_esc, base + macros, O.out + sidx);
    }
    if constexpr (HIERARCHY) {
      // the examination at the same boundary (uniform condition: it has barriers), until the system is resolved
      if (boundary && !resolved && r_sep > 0.f && S.n >= 2 && S.n <= kHierMax)
        resolved = batch_hierarchy_test<EXT>(S, (double)r_sep, (double)H.kappa, base + macros, H.rec + sidx,
                                             H.nodes + 2 * (size_t)first);
    }
  }
  if (threadIdx.x == 0) {
    BatchState* const bs = A.state + sidx;
    bs->block_steps += steps;
    bs->body_steps += bodies;
    bs->macro_steps += macros;
    if (steps != 0ull) bs->last_n_active = last_n;
    if (status != 0u) A.status[sidx] = status;
    if constexpr (EVENTS) {
      nbody_hip_batch_event_t e;
      // the conditions once more, so that the stop word is set by the launch in which they came to hold
      e.stopped = status == 0u && stopped == 0u ? stop_word() : stopped;
      e.reserved = 0u;
      e.macro_steps_done = base + macros;
      event_unkey(ckey, &e.closest_d2, &e.closest_i, &e.closest_j);
      e.closest_tick = ctick;
      e.closest_macro = cmacro;
      event_unkey(tkey, &e.contact_d2, &e.contact_i, &e.contact_j);
      e.contact_tick = ttick;
      e.contact_macro = tmacro;
      E.events[sidx] = e;
    }
  }
