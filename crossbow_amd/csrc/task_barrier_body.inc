// task_barrier_body.inc -- the body of the four fused task-step barrier
// kernels, included inside each of them behind its step policy `step`
// (task_barrier_step.h).  It is shared as text and not as a function: behind a
// call, even an inlined one, the compiler schedules the kernels differently,
// and their code objects are held fixed (DESIGN.md 10.2).
//
// For the same reason what one mode alone does is spelt out under
// `if constexpr` on the policy's constants, not hidden in helpers that do
// nothing for the other modes: those changed the plain kernel's code too.
//
// In scope: the kernel's template parameters R, MIXED, MOM, BMOM, WD, KEEP, P,
// TAIL, U, its parameter `a` (TaskBarrierArgs) and `step`.
//
// Per stepping replica i (one fp32 operation per reference call, in their
// order; built with -ffp-contract=off):
//   g = scale_i * g                                clipped only, before weight decay
//   g = fma(wd, w, g)                              sma.cu:24-31 (wd > 0)
//   s = w                                          :71 / :87
//   g = rate_i * g ; g = fma(mu, last_i, g) ; last_i = g ; w' = fma(1, g, w)   :52-74
//   or, without momentum, w' = fma(rate_i, g, w)   :90
// with r_iv = rate_i * mult[v] in place of rate_i where the rate is per
// variable (model.c:159-177); with a clip record's skip bit the step is s = w
// and nothing else: last_i and g_i are stored with the bits that were loaded,
// w' = w.  For a replica that only joins the barrier s = s_i, w' = w_i; then
// for all of them
//   d = fma(-1, z, s) ; w_i = fma(-alpha, d, w') ; acc = fma(alpha, d, acc)    sma.c:79-107
// and D = acc ; D = fma(0.9, last, D), last = D ; z = fma(1, D, z)             sma.c:148-174
// With a copy request (Phase D, sma.c:185-227) every w_i becomes the new z;
// last_i (and s_i, g_i) are written all the same.
{
  typedef decltype(step) STEP;
  constexpr int RR = (R > 0) ? R : kChunk;
  if constexpr (TAIL) {
    if (blockIdx.x < (uint32_t)a.tail_blocks) {
      task_barrier_tail_elem<MOM, BMOM, WD, KEEP>(a, step);
      return;
    }
  }
  const uint32_t tb = TAIL ? (uint32_t)a.tail_blocks : 0u;
  const uint32_t trip = (gridDim.x - tb) * blockDim.x * U;
  const uint32_t n4 = (uint32_t)a.n4;
  [[maybe_unused]] const uint32_t lane = threadIdx.x & 63u;
  const v4f al = a.alpha, nal = -a.alpha, mb = kBaseMomentum, one = 1.0f, mone = -1.0f;
  const v4f mu = a.momentum, wd = a.wd;
  const bool copy = a.copy != 0;
  for (uint32_t base = first_elem<U>(blockIdx.x - tb); base < n4; base += trip) {
    // Per variable, the lookup is per wave: a wave's 64 float4s are one
    // 256-float chunk of the host-built table (optimise_plan.h), at unroll 2
    // two chunks.  The wave's first chunk is wave-uniform, so the entries come
    // through scalar loads, issued with the trip's first float4 loads.
    [[maybe_unused]] uint32_t ch, e[U];
    [[maybe_unused]] v4f mv[U];
    if constexpr (STEP::kPerVariable) {
      ch = (uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 6));
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = step.chunks[ch + u];
    }
    v4f zv[U], lv[U], acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = (base + u * 64u) * 16u;
      zv[u] = ldo<P>(a.z, i);
      if constexpr (BMOM) lv[u] = ldo<P>(a.blast, i);
      acc[u] = 0.0f;  // sma.c:66
    }
    const int nrep = (R > 0) ? R : a.nrep;
    // one chunk's registers at a time: unrolled further, the mixed form spills
#pragma nounroll
    for (int c = 0; c < nrep; c += RR) {
      // a stepping replica: x = w, y = g, l = last_i; one that only joins: x = s, y = w
      v4f x[U][RR], y[U][RR], l[U][RR];
      [[maybe_unused]] v2u sf[RR];
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        if (R < 0 && c + r >= nrep) continue;  // a guard, not a break: the unrolled body keeps its registers
        const bool stepping = !MIXED || ((a.step_mask >> (c + r)) & 1ull) != 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (base + u * 64u) * 16u;
          // the stream is chosen by its (scalar) base, not by a branch around the
          // loads: branches here cost the mixed form its unrolled registers
          x[u][r] = ldo<P>(stepping ? a.w[c + r] : a.s[c + r], i);
          y[u][r] = ldo<P>(stepping ? a.g[c + r] : a.w[c + r], i);
          if constexpr (MOM) {
            if (stepping) l[u][r] = ldo<P>(a.last[c + r], i);
          }
        }
      }
      // The chunk's clip records, scale and flags of each in one 8-byte scalar
      // load, together and behind its float4 loads: no load waits for another,
      // and none is waited for ahead of the streams.
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
        // loads: the table entry is not waited for ahead of them.  In a chunk
        // with a boundary inside, each lane finds the variable of each of its
        // four floats in the sorted boundary array.
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
        // The offsets, made opaque here: the lookup's branches end the loads'
        // basic block, and an address carried over from it reaches the stores
        // as a 64-bit VGPR pair per stream; computed anew in this block it
        // folds into the "saddr + voffset" form again.
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
          v4f sv = x[u][r], wn;
          if (stepping) {
            // r_iv is a vector multiply of the (scalar) rate_i by the lane's four
            // multipliers: the same bits as a scalar multiply, and no branch here
            v4f rv = rate;
            if constexpr (STEP::kPerVariable) rv = rate * mv[u];
            v4f gv = y[u][r];
            if constexpr (STEP::kClips) gv = scale * y[u][r];
            if constexpr (WD) gv = vfma(wd, sv, gv);
            if constexpr (MOM) {
              gv = rv * gv;
              gv = vfma(mu, l[u][r], gv);
              if constexpr (STEP::kClips) sto<P>(a.last[c + r], i, pick(skip, l[u][r], gv));
              else sto<P>(a.last[c + r], i, gv);
              wn = vfma(one, gv, sv);
            } else {
              wn = vfma(rv, gv, sv);
            }
            if constexpr (STEP::kClips) wn = pick(skip, sv, wn);
            if constexpr (KEEP) {
              sto<P>(a.s[c + r], i, sv);
              if constexpr (STEP::kClips) sto<P>(a.g[c + r], i, pick(skip, y[u][r], gv));
              else if constexpr (MOM || WD) sto<P>(a.g[c + r], i, gv);
            }
          } else {
            wn = y[u][r];
          }
          const v4f d = vfma(mone, zv[u], sv);
          acc[u] = vfma(al, d, acc[u]);
          sto<P>(a.w[c + r], i, vfma(nal, d, wn));
        }
      }
      if constexpr (R > 0) break;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (base + u * 64u) * 16u;
      if constexpr (STEP::kPerVariable) asm volatile("" : "+v"(i));  // as `so` above
      v4f D = acc[u];
      if constexpr (BMOM) {
        D = vfma(mb, lv[u], D);
        sto<P>(a.blast, i, D);
      }
      zv[u] = vfma(one, D, zv[u]);
      sto<P>(a.z, i, zv[u]);
    }
    // Phase D is rare (a learning-rate boundary): the loop above stays free of
    // branches, and the lane's own later store to the same address wins.
    if (copy) {
      for (int r = 0; r < nrep; ++r) {
#pragma unroll
        for (int u = 0; u < U; ++u) sto<P>(a.w[r], (base + u * 64u) * 16u, zv[u]);
      }
    }
  }
}
