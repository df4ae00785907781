// task_elastic_policy_body.inc -- the body of the three fused task-step
// elastic-averaging kernels that have a step policy (task_elastic_variables_kernels.hip,
// task_elastic_clipped_kernels.hip, task_elastic_clipped_variables_kernels.hip),
// included inside each of them behind its policy `step` (task_barrier_step.h).
// It is task_elastic_kernel's loop (task_elastic_kernels.hip) with the policy
// members of task_barrier_body.inc, and shared as text for that file's reason.
//
// In scope: the kernel's template parameters R, MIXED, MOM, WD, KEEP, P, TAIL,
// U, its parameter `a` (TaskBarrierArgs) and `step`.
//
// Per participating replica i (one fp32 operation per reference call, in their
// order; built with -ffp-contract=off):
//   stepping:
//     g = scale_i * g                                clipped only, before weight decay
//     g = fma(wd, w, g)                              sma.cu:24-31 (wd > 0)
//     s = w                                          :71 / :87 (kept outputs only)
//     g = r * g ; g = fma(mu, last_i, g) ; last_i = g ; w' = fma(1, g, w)   :52-74
//     or, without momentum, w' = fma(r, g, w)        :90
//   with r = rate_i * mult[v] where the rate is per variable (model.c:159-177),
//   else rate_i; with a clip record's skip bit the step is s = w and nothing
//   else: last_i and g_i are stored with the bits that were loaded, w' = w_i.
//   only joining: w' = w_i
//   all: d = fma(-1, z, w') ; w_i = fma(-alpha, d, w') ; acc = fma(alpha, d, acc)   synchronouseamsgd.c:55-77
// then z = fma(1, acc, z) (:85-90), acc from +0 (:43).
{
  typedef decltype(step) STEP;
  constexpr int RR = (R > 0) ? R : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_elastic_policy_tail_elem<MOM, WD, KEEP>(a, step);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  [[maybe_unused]] const uint32_t lane = threadIdx.x & 63u;
  const v4f al = a.alpha, nal = -a.alpha, one = 1.0f, mone = -1.0f;
  const v4f mu = a.momentum, wd = a.wd;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    // Per variable, the lookup is per wave (task_barrier_body.inc): a wave's 64
    // float4s are one 256-float chunk of the host-built table, at unroll 2 two
    // chunks; the entries come through scalar loads, issued with the trip's
    // first float4 loads.
    [[maybe_unused]] uint32_t ch, e[U];
    [[maybe_unused]] v4f mv[U];
    if constexpr (STEP::kPerVariable) {
      ch = (uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 6));
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = step.chunks[ch + u];
    }
    v4f zv[U], acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      zv[u] = ldo<P>(a.z, (base + u * 64u) * 16u);
      acc[u] = 0.0f;  // synchronouseamsgd.c:43
    }
    const int nrep = (R > 0) ? R : a.nrep;
    // one chunk's registers at a time: unrolled further, the mixed form spills
#pragma nounroll
    for (int c = 0; c < nrep; c += RR) {
      // x = w_i; of a stepping replica also y = g_i and l = last_i
      v4f x[U][RR], y[U][RR], l[U][RR];
      [[maybe_unused]] v2u sf[RR];
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;  // a guard, not a break: the unrolled body keeps its registers
        const bool stepping = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          x[u][r] = ldo<P>(a.w[c + r], i);
          // a replica that only joins is this one stream: its g and last_i may not exist
          if (stepping) {
            y[u][r] = ldo<P>(a.g[c + r], i);
            if constexpr (MOM) l[u][r] = ldo<P>(a.last[c + r], i);
          }
        }
      }
      // The chunk's clip records, scale and flags of each in one 8-byte scalar
      // load, together and behind its float4 loads.  The entry of a replica
      // that only joins is loaded too and not used: the launcher has put a
      // valid record there (task_barrier_fill_records).
      if constexpr (STEP::kClips) {
#pragma unroll
        for (int r = 0; r < RR; ++r) {
          if (R < 0 && c + r >= nrep) continue;
          sf[r] = record_words(step.rec.p[c + r]);
        }
      }
      // every load of the chunk in flight before the first use (sma_fused_kernel)
      __builtin_amdgcn_sched_barrier(0);
      // byte offsets of the chunk's stores
      [[maybe_unused]] uint32_t so[U];
      if constexpr (STEP::kPerVariable) {
        // The multipliers, once per trip and behind the first replica chunk's
        // loads.  In a chunk with a boundary inside, each lane finds the
        // variable of each of its four floats in the sorted boundary array.
        if (R > 0 || c == 0) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const uint32_t v0 = e[u] >> 1;
            if ((e[u] & 1u) == 0u) {    // wave-uniform
              mv[u] = step.mult[v0];  // a scalar load
            } else {
              const uint32_t f = (ch + u) * kOptChunk + lane * 4u;
#pragma unroll
              for (int k = 0; k < 4; ++k) mv[u][k] = step.mult[variable_of(step.bounds, step.nvars, v0, f + k)];
            }
          }
        }
        // The offsets, made opaque after the lookup's branches: computed anew
        // in this block they fold into the "saddr + voffset" form again
        // (task_barrier_body.inc).
#pragma unroll
        for (int u = 0; u < U; ++u) {
          so[u] = (base + u * 64u) * 16u;
          asm volatile("" : "+v"(so[u]));
        }
      }
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;
        const bool stepping = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
        const v4f rate = a.rate[c + r];
        [[maybe_unused]] v4f scale;
        [[maybe_unused]] bool skip = false;  // wave-uniform
        if constexpr (STEP::kClips) {
          scale = __uint_as_float(sf[r][0]);
          skip = (sf[r][1] & kClipSkipped) != 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          uint32_t i = (base + u * 64u) * 16u;
          if constexpr (STEP::kPerVariable) i = so[u];
          const v4f wv = x[u][r];
          v4f wn = wv;
          if (stepping) {
            // r_iv: a vector multiply of the (scalar) rate_i by the lane's four multipliers
            v4f rv = rate;
            if constexpr (STEP::kPerVariable) rv = rate * mv[u];
            v4f gv = y[u][r];
            if constexpr (STEP::kClips) gv = scale * y[u][r];
            if constexpr (WD) gv = vfma(wd, wv, gv);
            if constexpr (MOM) {
              gv = rv * gv;
              gv = vfma(mu, l[u][r], gv);
              if constexpr (STEP::kClips) sto<P>(a.last[c + r], i, pick(skip, l[u][r], gv));
              else sto<P>(a.last[c + r], i, gv);
              wn = vfma(one, gv, wv);
            } else {
              wn = vfma(rv, gv, wv);
            }
            if constexpr (STEP::kClips) wn = pick(skip, wv, wn);
            if constexpr (KEEP) {
              sto<P>(a.s[c + r], i, wv);
              if constexpr (STEP::kClips) sto<P>(a.g[c + r], i, pick(skip, y[u][r], gv));
              else if constexpr (MOM || WD) sto<P>(a.g[c + r], i, gv);
            }
          }
          const v4f d = vfma(mone, zv[u], wn);
          sto<P>(a.w[c + r], i, vfma(nal, d, wn));
          acc[u] = vfma(al, d, acc[u]);
        }
      }
      if constexpr (R > 0) break;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (base + u * 64u) * 16u;
      if constexpr (STEP::kPerVariable) asm volatile("" : "+v"(i));  // as `so` above
      sto<P>(a.z, i, vfma(one, acc[u], zv[u]));
    }
  }
}
