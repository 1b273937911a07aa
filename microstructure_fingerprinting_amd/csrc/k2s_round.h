// k2s_round.h -- the body of ONE round of mfx_fit_k2s_kernel (fit_k2s.hip), included as plain text inside a `for (int round ...)`
// loop of the kernel (no include guard: fit_k2s.hip includes it once per K2S_ROUND_MODE), in the scope of the kernel's locals.
// K2S_ROUND_MODE 0: whether the round is the shared last row tile is decided at run time; 1: it is; 2: it is not.
    // A last round with ONE row tile left (N = 782: 25 = 3*8 + 1) is shared by all waves: each keeps the same
    // A tile and takes every 8th column tile, generating its B operand straight into registers (no LDS image,
    // no workgroup barrier), instead of 7 waves idling through a full D2 sweep.
    const bool tail = K2S_ROUND_MODE == 0 ? (ntiles - round * NW == 1) && (ntiles > 1) : K2S_ROUND_MODE == 1;
    const int rt = tail ? round * NW : round * NW + wave;
    const bool rt_valid = rt < ntiles;  // wave-uniform
    const int rtc = rt_valid ? rt : 0;
    // A operand: this wave's 32 atoms of D1, all KS k-steps, split in registers - UN-normalised like D2 (the table
    // is pre-scaled to values <= 128), so that the column statistics I1 = 1/|d1|, Z1 = d1.y/|d1| fall out of the
    // same read of the table (ranking only, as in phase 1; a lane sums its half of the rows, the halves meet
    // through one cross-lane exchange): the L2 -> L1 fill rate bounds these passes, not the arithmetic.
    h8 afh[KS], afl[KS];
#if K2S_ROUND_MODE == 1
    // 16-ROW FORM (the fused pass only): a last row tile with at most 16 atoms (N = 782: 14) runs on v_mfma_f32_16x16x32_f16;
    // its A operand is made where it is used, in the tail branch below
    const bool t16 = N - 32 * (ntiles - 1) <= 16;   // wave-uniform
    if (!t16)
#endif
    {
      const int n = rtc * 32 + lr;
      const int nn = min(n, ldn - 1);
      double a2 = 0.0, ay = 0.0;
      // XC: the LAST padded measurement row (MP - 1 > M - 1: the launcher sees to that; the table's padded rows are
      // zero) carries -u1 in the A operand and u2 in the B images - a compile-time position: a test against M per element
      // is loop-invariant, gets hoisted out of the rounds and costs ~100 spilled registers
      float um1 = 0.0f;
      if constexpr (XC) um1 = (rt_valid && n < N) ? -s_uf[n] : 0.0f;
      mfx_static_for<0, KS>([&](auto kc) {
        constexpr int ks = decltype(kc)::value;
        float2 d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = tab32_at(s_rs[16 * ks + 8 * lh + j], nn);
        h8 vh, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float fv = fmaf(d[j].y, s_t0f[16 * ks + 8 * lh + j], d[j].x);
          fv = rt_valid ? fv : 0.0f;
          if constexpr (XC) {
            if constexpr (ks == KS - 1) { if (j == 7) fv = lh ? um1 : fv; }
          } else {
            const double fd = (double)fv;
            a2 = fma(fd, fd, a2);
            ay = fma((double)s_yf[16 * ks + 8 * lh + j], fd, ay);
          }
          _Float16 x, y;
          mfx_split16(fv, x, y);
          vh[j] = x; vl[j] = y;
        }
        asm volatile("" : "+v"(vh), "+v"(vl));   // materialise here: the conversions must not sink below all loads
        afh[ks] = vh; afl[ks] = vl;
        __builtin_amdgcn_sched_barrier(0);
      });
      if constexpr (!XC) {   // (XC: the statistics of both dictionaries come from phase 1, and one-atom supports are not this kernel's)
      a2 += __shfl_xor(a2, 32);
      ay += __shfl_xor(ay, 32);
      const bool act = rt_valid && n < N;
      const double nrm = sqrt(a2);
      const double inv = (act && a2 > 0.0) ? 1.0 / nrm : 0.0;
      const double z = ay * inv;
      if (rt_valid && lh == 0) {
        s_Zf[n] = act ? (float)z : -1e30f;
        s_cs[n] = (act && a2 > 0.0) ? (float)nrm : 0.0f;
      }
      // best single-atom score of this row tile (the atoms themselves join the candidates in k2s_finish, from s_Zf)
      double sb = (act && z > 0.0) ? z * z : 0.0;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sb = fmax(sb, __shfl_xor(sb, o));
      sb = mfx_readlane_f64(sb, 0);
      // a pair matters only if it beats every single atom
      if (lane == 0 && sb - mrg > 0.0) atomicMax(&s_thr[0], mfx_nonneg_bits(sb - mrg));
      }
    }

    // pair screen of one 32x32 accumulator tile against column tile ct (used by the LDS sweep and by the tail round)
    //
    // Fast pass in FP32, 3 VALU per pair.  With unit atoms at angle phi (c = cos phi), the projection of y on
    // their plane has squared length S and makes the angles alpha1, alpha2 with them (z_i = sqrt(S) cos alpha_i);
    // both weights are positive exactly when it lies between the atoms: phi = alpha1 + alpha2.  For any T <= S,
    // theta_i = acos(min(1, max(z_i, 0) / sqrt(T))) <= alpha_i, hence
    //     two positive weights and S >= T   ==>   c <= cos(theta1 + theta2) = P1 P2 - Q1 Q2,
    // P_i = cos theta_i, Q_i = sin theta_i (the other branch of S(c) >= T, c >= cos(theta1 - theta2), has a
    // non-positive weight).  The test is therefore  c~ - DC <= P1 P2 - Q1 Q2  with T = the running threshold;
    // a STALE (lower) threshold, P rounded up and Q rounded down only let more pairs through.  In accumulator
    // units (acc = c |d1| |d2|, neither operand is normalised) the margin is folded into the constants,
    //     (P1 + D)(P2 + D) - (1 - D)^2 Q1 Q2  >=  P1 P2 - Q1 Q2 + D      for all P, Q = sqrt(1 - P^2) in [0, 1]
    // (the difference is D (P1 + P2 + (2 - D) Q1 Q2 - 1) + D^2 and P1 + P2 + 1.99 Q1 Q2 >= 1 on the unit square),
    // at the price of a margin up to ~3 D instead of D:
    //     t = ((P1 + D) n1)((P2 + D) n2) - ((1 - D) Q1 n1)((1 - D) Q2 n2) - acc,      pass when max t >= 0:
    // two FMAs and a max per pair, from two constants per row and two per column.  Rows and columns beyond N get
    // constants that do not pass (but for the corner cases noted below).  Only a register group with a passing
    // pair runs the FP64 criteria below (one out-of-line copy).
    double thr = 0.0, thr_rows = -1.0;
#ifdef MFX_STAMPS_RND
    int dbg_flagged = 0, dbg_groups = 0;   // accumulator tiles / register groups of this wave that reached the FP64 criteria
#endif
    const float DCF = XC ? (float)((mfx_s_dc<KS>() + 2e-6) * ramp) * (1.0f + 2e-7f)
                         : (float)mfx_s_dc<KS>() + 2e-6f;   // + the FP32 evaluation error of t (< 1e-6 in cosine units)
    auto pq_of = [&](float z, float rth, float& P, float& Q) {
      P = fminf(1.0f, fmaxf(z, 0.0f) * rth);
      Q = __builtin_amdgcn_sqrtf(fmaxf(0.0f, fmaf(-P, P, 1.0f) - 1.2e-7f)) * (1.0f - 3e-7f);
    };
    // scan_pre only ISSUES the LDS reads of a tile's column (threshold, column statistics): a screening wave has
    // no partner to cover an LDS round trip, so they fly behind the generation work; scan_main does the rest
    unsigned long long sc_thr = 0ull;
    float sc_z2 = 0.0f, sc_s = 0.0f;
    auto scan_pre = [&](int ct) {
      const int j = ct * 32 + lr;
      sc_thr = s_thr[0];
      sc_z2 = s_Zf[NP + j];
      sc_s = s_cs[NP + j];
    };
#ifdef MFX_STAMPS_SCAN   // diagnostic builds: wave 0's first pair screen of a voxel in detail (tools/dev_stamps_scan.py)
    int dbg_calls = 0;
#define MFX_SCAN_T(k) do { if (a.stamps && round == 0 && dbg_calls == 1 && wave == 0 && lane == 0) a.stamps[(size_t)blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define MFX_SCAN_T(k) do { } while (0)
#endif
    // the FP64 criteria of ONE register group with a passing pair: row atom i, column atom j (per lane), the raw accumulator
    // value and the column statistics.  One out-of-line copy for the sweeps, the shared tile and its 16-row form.
    auto scan_pair = [&](const int i, const int j, const float accv, const double z2, const double n2d) {
      const double n12 = (double)s_cs[i] * n2d;
      const double c = n12 > 0.0 ? (double)accv * mfx_rcp_nr(n12) : 0.0;
      const double z1 = (double)s_Zf[i];
      const double e1 = fma(-c, z2, z1);
      const double e2 = fma(-c, z1, z2);
      const double den = fma(-c, c, 1.0);
      const double num = fma(z2, e2, z1 * e1);
      const bool pos = (e1 > -etol) & (e2 > -etol);      // false for padded atoms (z = -inf)
      // (dS/dc = -2 w1 w2 <= |y|^2 needs c >= 0; pairs at an obtuse angle - no physical dictionary has them -
      // go through the interval bound like the ill-conditioned ones)
      const bool wellc = (den >= MFX_S_DENMIN) & (c >= 0.0);
      const bool hit = pos & wellc & (fma(-thr, den, num) >= 0.0);
      const bool near = pos & !wellc;
      if (!__any(hit | near)) return;
      double S = -1.0;
      if (hit) {
        S = num * mfx_rcp_nr(den);
      } else if (near) {
        // ill-conditioned pair: interval upper bound of S over |c - c~| <= DC;
        // S = z2^2 + e1^2/den = z1^2 + e2^2/den for two positive weights
        const double dlo = den - 2.0 * dc_eff - dc_eff * dc_eff;
        const double u1 = fabs(e1) + etol, u2 = fabs(e2) + etol;
        S = (dlo > 0.0 && c > -0.5) ? fmin(fma(z2, z2, u1 * u1 / dlo), fma(z1, z1, u2 * u2 / dlo)) + mrg : 1e300;
      }
      // raise the threshold with the best SCORE of this wave instruction first (an interval bound is not
      // a score and never raises it), then append only what still reaches it: no burst of stale entries
      bool feas = hit;
      double q1x = 0.0, q2x = 0.0;   // (XC) u / |d'| of the two atoms
      if constexpr (XC) {
        // a relaxed score may raise the threshold only if it is the score of a feasible support: x's weight
        // w_x = yx - w1 u1 - w2 u2, w_i = e_i / (den |d_i'|), clearly non-negative (e carries an error <= etol,
        // u/|d'| <= 4)
        q1x = (double)s_uf[i] * mfx_rcp_nr(fmax((double)s_cs[i], 1e-300));
        q2x = (double)s_uf[NP + j] * mfx_rcp_nr(fmax(n2d, 1e-300));
        feas = hit && (fma(-e2, q2x, fma(-e1, q1x, yx * den)) >= 8.0 * etol);
      }
      double sraise = feas ? S : 0.0;
      double slist = S;   // what the pair is listed with: an upper bound of the best score of its supports with BOTH atoms
      if constexpr (XC) {
        // x would get a negative weight: the pair's PLAIN two-atom score (x left out) is feasible and raises the
        // threshold instead - without it a voxel with no x signal never leaves the single-atom threshold, floods
        // the ring and ends up on the FP64 kernel.  Unprojected statistics from the projected ones:
        // |d|^2 = |d'|^2 + u^2, d.y = z' |d'| + u yx, d1.d2 = d1'.d2' + u1 u2; scores here are minus yx^2.
        if (__any(hit && !feas)) {
          const double n1p = (double)s_cs[i], u1 = (double)s_uf[i], u2 = (double)s_uf[NP + j];
          const double m1 = fma(u1, u1, n1p * n1p), m2 = fma(u2, u2, n2d * n2d);
          const double i1 = mfx_rcp_nr(fmax(sqrt(m1), 1e-300)), i2 = mfx_rcp_nr(fmax(sqrt(m2), 1e-300));
          const double w1 = fma(u1, yx, z1 * n1p) * i1, w2 = fma(u2, yx, z2 * n2d) * i2;   // d.y / |d|
          const double c0 = fma(u1, u2, (double)accv) * i1 * i2;
          const double f1 = fma(-c0, w2, w1), f2 = fma(-c0, w1, w2), den0 = fma(-c0, c0, 1.0);
          const bool ok0 = hit && !feas && (f1 > etol) && (f2 > etol) && (den0 >= MFX_S_DENMIN) && (c0 >= 0.0) && (m1 > 0.0) && (m2 > 0.0);
          if (ok0) sraise = fma(w2, f2, w1 * f1) * mfx_rcp_nr(den0) - yx * yx;
          // A pair whose relaxed optimum CLEARLY gives x a negative weight (both atoms clearly active in it) has x
          // inactive in its NNLS optimum: that optimum is the plain two-atom problem's.  Listed with the plain score
          // then, or - one atom clearly inactive there - not at all (supports with one atom are the list kernel's
          // own).  Without this a flagged voxel WITHOUT x signal lists every pair its loose relaxed bound lets
          // through: 17 % of such voxels overflowed their list and went to the FP64 kernel.
          const bool xneg = hit && (e1 > etol) && (e2 > etol) && (fma(-e2, q2x, fma(-e1, q1x, yx * den)) <= -8.0 * etol) &&
                            (den0 >= MFX_S_DENMIN) && (c0 >= 0.0) && (m1 > 0.0) && (m2 > 0.0);
          if (xneg) {
            if (ok0) slist = sraise + mrg;
            else if (f1 < -etol || f2 < -etol) slist = -1.0;
          }
        }
      }
      const double smax = mfx_wave_max_down(fmax(sraise, 0.0));
      if (smax - 2.0 * mrg > thr) {
        thr = smax - 2.0 * mrg;
        if (lane == 0) atomicMax(&s_thr[0], mfx_nonneg_bits(thr));
      }
      if ((hit | near) && slist >= thr) push(slist, i, hit ? j : (j | MFX_S_BOUND));
#ifdef MFX_STAMPS_SCAN
      if (a.stamps && round == 0 && dbg_calls == 1 && wave == 0 && lane == 0) {
        unsigned long long* st = a.stamps + (size_t)blockIdx.x * 16;
        if (st[15] < 8) st[4 + st[15]] = __builtin_amdgcn_s_memtime();   // end of the first 8 evaluated groups
        ++st[15];
      }
#endif
    };
    auto scan_main = [&](const f32x16& acc, int ct) {
#ifdef MFX_STAMPS_SCAN
      ++dbg_calls;
#endif
      MFX_SCAN_T(0);
      {
        if (((rt << 8) | ct) == aud_key) {   // once per voxel, one wave: park the raw accumulator value of the audited pair (k2s_shared.h)
          const unsigned h = k2s_audit_hash(vox);
          const int ga = (h >> 16) & 15;
          float v = acc[0];
#pragma unroll
          for (int g = 1; g < 16; ++g) v = (ga == g) ? acc[g] : v;
          if (lane == (int)((h >> 20) & 63)) ((float*)(s_red + 30))[0] = v;
        }
      }
      const int j = ct * 32 + lr;
      // row i = rt*32 + (g&3) + 8(g>>2) + 4 lh, column j = ct*32 + lr
      thr = fmax(thr, __longlong_as_double((long long)sc_thr));
      // 1/sqrt(T), T = thr rounded down, the reciprocal root rounded up (v_rsq_f32: 1 ulp)
      const float rth = __builtin_amdgcn_rsqf(fmaxf((float)thr * (1.0f - 2e-7f), 1e-30f)) * (1.0f + 4e-7f);
      float* pqw = s_pq + wave * 64;
      if (thr > thr_rows) {   // wave-uniform: the threshold rose since this wave's row constants were made
        thr_rows = thr;
        if (lane < 32) {
          const float z1 = s_Zf[rtc * 32 + lane], n1 = s_cs[rtc * 32 + lane];
          float P, Q;
          pq_of(z1, rth, P, Q);
          // beyond N: (0, 1e18) for rows, (-1e18, 1e18) for columns: t < 0 but for a padded row against a column
          // with Q2 = 0 (its atom alone reaches the threshold), which the FP64 criteria reject
          const bool ok = n1 > 0.0f;
          pqw[lane] = ok ? (P + DCF) * n1 : 0.0f;
          pqw[32 + lane] = ok ? Q * ((1.0f - DCF) * n1) : 1e18f;
        }
      }
      const float z2f = sc_z2, n2 = sc_s;
      float P2, Q2;
      pq_of(z2f, rth, P2, Q2);
      const bool colok = n2 > 0.0f;
      const float p2 = colok ? (P2 + DCF) * n2 : -1e18f, q2 = colok ? Q2 * ((1.0f - DCF) * n2) : 1e18f;
      float mm[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 p1q = *(const f32x4*)(pqw + 8 * q + 4 * lh);        // rows (g&3) + 8q + 4 lh, g = 4q..4q+3
        const f32x4 q1q = *(const f32x4*)(pqw + 32 + 8 * q + 4 * lh);
        // plain (not packed) FP32: beside the other wave's MFMAs a v_pk_*_f32 costs several plain ones
        float t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = fmaf(-q1q[u], q2, fmaf(p1q[u], p2, -acc[4 * q + u]));
        mm[q] = fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3]));
      }
      MFX_SCAN_T(1);
      if (__any(fmaxf(fmaxf(mm[0], mm[1]), fmaxf(mm[2], mm[3])) >= 0.0f)) {
        MFX_SCAN_T(2);
#ifdef MFX_STAMPS_RND
        ++dbg_flagged;
#endif
        // ---- exact FP64 pass over the flagged register groups (rare once thr is close to the optimum)
        // the column statistics are ranking-grade anyway (FP32 table): their FP32 copies serve here too
        // (6e-8 relative: ~4e-7 |y|^2 in a score, against the margin of 1e-5 |y|^2)
        const double z2 = (double)s_Zf[NP + j], n2d = (double)s_cs[NP + j];
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
          if (!__any(mm[q] >= 0.0f)) continue;
          // the quad's four register groups one by one: the FP32 test again (mm[q] is their maximum), so that only
          // groups with a passing pair pay the ~40 FP64 instructions below - the seven other waves of the workgroup
          // wait at the period's barrier for a wave that is in here
          const f32x4 p1q = *(const f32x4*)(pqw + 8 * q + 4 * lh);
          const f32x4 q1q = *(const f32x4*)(pqw + 32 + 8 * q + 4 * lh);
#pragma unroll 1
          for (int gg = 0; gg < 4; ++gg) {
            const int g = 4 * q + gg;
            if (!__any(fmaf(-q1q[gg], q2, fmaf(p1q[gg], p2, -acc[g])) >= 0.0f)) continue;
#ifdef MFX_STAMPS_RND
            ++dbg_groups;
#endif
            scan_pair(rt * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh, j, acc[g], z2, n2d);
          }
        }
        MFX_SCAN_T(3);
      }
    };
    auto scan_tile = [&](const f32x16& acc, int ct) { scan_pre(ct); scan_main(acc, ct); };

#ifdef MFX_EXP_NOTAIL   // timing experiment (wrong results): what the shared last row tile costs
    if (tail) continue;
#endif
    if (tail) {
#if K2S_ROUND_MODE == 1
      if (!t16)
#endif
      {
#ifdef MFX_STAMPS_RND
      if (a.stamps && tid == 0 && round < 4) a.stamps[(size_t)blockIdx.x * 16 + 2 * round + 1] = __builtin_amdgcn_s_memtime();
#endif
      thr = __longlong_as_double((long long)s_thr[0]);
      }
      // (!XC: the fused pass) D2's statistics from the values that make the B operand, as the A-operand code does for D1:
      // a lane sums its half of the rows of column n in FP64, the halves meet through one cross-lane exchange.  The wave
      // then owns the statistics of its column tiles: it writes them, folds them into its best single atom of D2 and into
      // the threshold, and only THEN screens the tile (with thr = 0 the fast test passes every pair).
      // best single atom of D2 among this wave's column tiles (first index on ties): kept in the wave's slot of s_red, where
      // k2s_best_single_late looks for it, not in registers carried through the pass
      [[maybe_unused]] double* const s_bs2 = s_red + 8 + wave;
      [[maybe_unused]] int* const s_bn2 = (int*)(s_red + 16) + 8 + wave;
      if constexpr (!XC) { if (lane == 0) { *s_bs2 = 0.0; *s_bn2 = 0; } }
#if K2S_ROUND_MODE == 1
      if (t16) {
        // 16-ROW FORM (the fused pass only): a last row tile with at most 16 atoms (N = 782: 14) runs on v_mfma_f32_16x16x32_f16,
        // index maps in k2s_tail16_map.h.  Lane 16 g + c holds the rows 32 s + 8 g + j of step s: of atom c of the tile here,
        // of the two adjacent atoms 2c, 2c+1 of a column tile - ONE 16-byte table load each - in the column loop below.  Half
        // the A registers and wave loads of the 32-row form, whose rows 16..31 would all be zeros.
        constexpr int NS16 = k2s_t16_steps(KS);
        const int g16 = lane >> 4;   // lane group
        h8 a16h[NS16], a16l[NS16];
        {   // A operand and D1's statistics of the tile, as at the top of the round for 32 rows
          const int n = rtc * 32 + k2s_t16_arow(lane);
          const int nn = min(n, ldn - 1);
          double a2 = 0.0, ay = 0.0;
          mfx_static_for<0, NS16>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            // (odd KS, last step: the lane groups 2 and 3 lie beyond MP - zeros, and the constants of rows that exist)
            const int m0 = k2s_t16_row(lane, 0, s, KS);
            const bool inr = m0 >= 0;
            const int mb = inr ? m0 : 32 * s;
            float2 d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = tab32_at(s_rs[mb + j], nn);
            h8 vh, vl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float fv = fmaf(d[j].y, s_t0f[mb + j], d[j].x);
              fv = inr ? fv : 0.0f;
              const double fd = (double)fv;
              a2 = fma(fd, fd, a2);
              ay = fma((double)s_yf[mb + j], fd, ay);
              _Float16 x, y;
              mfx_split16(fv, x, y);
              vh[j] = x; vl[j] = y;
            }
            asm volatile("" : "+v"(vh), "+v"(vl));   // materialise here: the conversions must not sink below all loads
            a16h[s] = vh; a16l[s] = vl;
            __builtin_amdgcn_sched_barrier(0);
          });
          // the four lane groups hold a quarter of the rows each: two exchanges, the same value in all four
          a2 += __shfl_xor(a2, 16); ay += __shfl_xor(ay, 16);
          a2 += __shfl_xor(a2, 32); ay += __shfl_xor(ay, 32);
          const bool act = n < N;
          const double nrm = sqrt(a2);
          const double inv = (act && a2 > 0.0) ? 1.0 / nrm : 0.0;
          const double z = ay * inv;
          if (g16 == 0) {
            s_Zf[n] = act ? (float)z : -1e30f;
            s_cs[n] = (act && a2 > 0.0) ? (float)nrm : 0.0f;
          } else if (g16 == 1) {   // slots 16..31 of the tile: no such atoms
            s_Zf[n + 16] = -1e30f;
            s_cs[n + 16] = 0.0f;
          }
          double sb = (act && z > 0.0) ? z * z : 0.0;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) sb = fmax(sb, __shfl_xor(sb, o));
          sb = mfx_readlane_f64(sb, 0);
          // a pair matters only if it beats every single atom
          if (lane == 0 && sb - mrg > 0.0) atomicMax(&s_thr[0], mfx_nonneg_bits(sb - mrg));
        }
#ifdef MFX_STAMPS_RND
        if (a.stamps && tid == 0 && round < 4) a.stamps[(size_t)blockIdx.x * 16 + 2 * round + 1] = __builtin_amdgcn_s_memtime();
#endif
        thr = __longlong_as_double((long long)s_thr[0]);
        // ---- 16-row form of the column loop: the 32 atoms of a column tile as two 16-column sub-tiles, the even atoms
        // (sub-tile 0) and the odd ones (1); a lane's 16-byte load {ylo, slope} x 2 feeds its own column of both.
        for (int ct = wave; ct < ntiles; ct += NW) {
          const int n0 = ct * 32 + k2s_t16_atom(lane, 0);   // this lane's atoms: n0 (sub-tile 0), n0 + 1 (sub-tile 1)
          const int nn = min(n0, ldn - 2);                  // ldn is even: the pair stays inside the row
          double a2[2] = {0.0, 0.0}, ay[2] = {0.0, 0.0};
          f32x4 acc16[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) acc16[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          f32x4 d[2][8];   // table entries of step s (in use) and s + 1 (in flight)
          {
            const int mb = MP + k2s_t16_row(lane, 0, 0, KS);   // (step 0 lies inside MP for every KS >= 2)
#pragma unroll
            for (int j = 0; j < 8; ++j) d[0][j] = tab32x2_at(s_rs[mb + j], nn);
          }
          static_assert(KS >= 2, "step 0 of the 16-row form must lie inside MP");
          mfx_static_for<0, NS16>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            int lk = lane;   // (bracketed rows: an opaque copy per step keeps each LDS address next to its use, as in the 32-row form)
            if constexpr (BR) asm volatile("" : "+v"(lk));
            if constexpr (s + 1 < NS16) {
              const int m1 = k2s_t16_row(lk, 0, s + 1, KS);
              const int mb1 = MP + (m1 >= 0 ? m1 : 32 * (s + 1));
#pragma unroll
              for (int j = 0; j < 8; ++j) d[(s + 1) & 1][j] = tab32x2_at(s_rs[mb1 + j], nn);
            }
            const int m0 = k2s_t16_row(lk, 0, s, KS);
            const bool inr = m0 >= 0;
            const int mb = inr ? m0 : 32 * s;
            h8 bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float t0 = s_t0f[MP + mb + j];
              const double yj = (double)s_yf[mb + j];
              const f32x4 e = d[s & 1][j];
              float fv[2] = {fmaf(e[1], t0, e[0]), fmaf(e[3], t0, e[2])};
#pragma unroll
              for (int t = 0; t < 2; ++t) {
                fv[t] = inr ? fv[t] : 0.0f;
                const double fd = (double)fv[t];
                a2[t] = fma(fd, fd, a2[t]);
                ay[t] = fma(yj, fd, ay[t]);
                _Float16 x, y;
                mfx_split16(fv[t], x, y);
                bh[t][j] = x; bl[t][j] = y;
              }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              acc16[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16h[s], bh[t], acc16[t], 0, 0, 0);
              acc16[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16h[s], bl[t], acc16[t], 0, 0, 0);
              acc16[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16l[s], bh[t], acc16[t], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
          });
          // column statistics: the four lane groups hold a quarter of the rows each
          float zf[2], nf[2];
          double sbt[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            a2[t] += __shfl_xor(a2[t], 16); ay[t] += __shfl_xor(ay[t], 16);
            a2[t] += __shfl_xor(a2[t], 32); ay[t] += __shfl_xor(ay[t], 32);
            const bool act = n0 + t < N;
            const double nrm = sqrt(a2[t]);
            const double inv = (act && a2[t] > 0.0) ? 1.0 / nrm : 0.0;
            const double z = ay[t] * inv;
            zf[t] = act ? (float)z : -1e30f;
            nf[t] = (act && a2[t] > 0.0) ? (float)nrm : 0.0f;
            sbt[t] = (act && z > 0.0) ? z * z : 0.0;
          }
          if (g16 == 0) {   // (all four groups hold the same values)
            *(float2*)(s_Zf + NP + n0) = float2{zf[0], zf[1]};
            *(float2*)(s_cs + NP + n0) = float2{nf[0], nf[1]};
          }
          double sb = sbt[0];
          int nb = n0;
          if (sbt[1] > sb) { sb = sbt[1]; nb = n0 + 1; }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) {
            const double s2 = __shfl_xor(sb, o);
            const int n2 = __shfl_xor(nb, o);
            const bool take = (s2 > sb) || (s2 == sb && n2 < nb);
            sb = take ? s2 : sb;
            nb = take ? n2 : nb;
          }
          sb = mfx_readlane_f64(sb, 0);
          nb = __builtin_amdgcn_readfirstlane(nb);
          if (lane == 0) {
            const double b2 = *s_bs2;
            if (sb > b2 || (sb == b2 && sb > 0.0 && nb < *s_bn2)) { *s_bs2 = sb; *s_bn2 = nb; }
          }
          // a pair matters only if it beats every single atom: the threshold rises BEFORE the tile is screened
          if (lane == 0 && sb - mrg > 0.0) atomicMax(&s_thr[0], mfx_nonneg_bits(sb - mrg));
          __builtin_amdgcn_wave_barrier();
          // ---- pair screen of the two 16x16 accumulator tiles: the test of scan_main, row i = rt*32 + 4 g + r, column n0 + t
          thr = fmax(thr, __longlong_as_double((long long)s_thr[0]));
          const float rth = __builtin_amdgcn_rsqf(fmaxf((float)thr * (1.0f - 2e-7f), 1e-30f)) * (1.0f + 4e-7f);
          float* pqw = s_pq + wave * 64;   // [0..15] P', [16..31] Q' of the 16 rows
          if (thr > thr_rows) {   // wave-uniform: the threshold rose since this wave's row constants were made
            thr_rows = thr;
            if (lane < 16) {
              const float z1 = s_Zf[rtc * 32 + lane], n1 = s_cs[rtc * 32 + lane];
              float P, Q;
              pq_of(z1, rth, P, Q);
              const bool ok = n1 > 0.0f;   // (beyond N: constants that do not pass, as in scan_main)
              pqw[lane] = ok ? (P + DCF) * n1 : 0.0f;
              pqw[16 + lane] = ok ? Q * ((1.0f - DCF) * n1) : 1e18f;
            }
          }
          const f32x4 p1 = *(const f32x4*)(pqw + 4 * g16), q1 = *(const f32x4*)(pqw + 16 + 4 * g16);
          float p2[2], q2[2], mm[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            float P2, Q2;
            pq_of(zf[t], rth, P2, Q2);
            const bool colok = nf[t] > 0.0f;
            p2[t] = colok ? (P2 + DCF) * nf[t] : -1e18f;
            q2[t] = colok ? Q2 * ((1.0f - DCF) * nf[t]) : 1e18f;
            float tt[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) tt[r] = fmaf(-q1[r], q2[t], fmaf(p1[r], p2[t], -acc16[t][r]));
            mm[t] = fmaxf(fmaxf(tt[0], tt[1]), fmaxf(tt[2], tt[3]));
          }
          if (__any(fmaxf(mm[0], mm[1]) >= 0.0f)) {
#ifdef MFX_STAMPS_RND
            ++dbg_flagged;
#endif
#pragma unroll 1
            for (int u = 0; u < 8; ++u) {   // register group u = 4 t + r, one by one as in scan_main
              const int t = u >> 2, r = u & 3;
              const float av = t ? acc16[1][r] : acc16[0][r];
              const float p2t = t ? p2[1] : p2[0], q2t = t ? q2[1] : q2[0];
              if (!__any(fmaf(-q1[r], q2t, fmaf(p1[r], p2t, -av)) >= 0.0f)) continue;
#ifdef MFX_STAMPS_RND
              ++dbg_groups;
#endif
              scan_pair(rt * 32 + k2s_t16_crow(lane, r), n0 + t, av, (double)(t ? zf[1] : zf[0]), (double)(t ? nf[1] : nf[0]));
            }
          }
        }
      } else
#endif
      for (int ct = wave; ct < ntiles; ct += NW) {
        const int n = ct * 32 + lr;
        const int nn = min(n, ldn - 1);
        float tail_u2 = 0.0f;
        if constexpr (XC) tail_u2 = s_uf[NP + n];
        [[maybe_unused]] double a2 = 0.0, ay = 0.0;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
        float2 d[2][8];   // table entries of k-step ks (in use) and ks+1 (in flight)
#pragma unroll
        for (int j = 0; j < 8; ++j) d[0][j] = tab32_at(s_rs[MP + 8 * lh + j], nn);
        mfx_static_for<0, KS>([&](auto kc) {
          constexpr int ks = decltype(kc)::value;
          // (bracketed rows, fused pass: the LDS addresses of every k-step's constants, hoisted out of the column loop, are
          // what the register file has no room for beside the statistics - an opaque copy of the lane half per k-step
          // keeps each address next to its use)
          int lhk = lh;
          if constexpr (BR && !XC) asm volatile("" : "+v"(lhk));
          if constexpr (ks + 1 < KS) {
#pragma unroll
            for (int j = 0; j < 8; ++j) d[(ks + 1) & 1][j] = tab32_at(s_rs[MP + 16 * (ks + 1) + 8 * lhk + j], nn);
          }
          h8 bh, bl;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            _Float16 x, y;
            float fv = fmaf(d[ks & 1][j].y, s_t0f[MP + 16 * ks + 8 * lhk + j], d[ks & 1][j].x);
            if constexpr (XC && ks == KS - 1) { if (j == 7) fv = lh ? tail_u2 : fv; }   // the spare row carries u2
            if constexpr (!XC) {
              const double fd = (double)fv;
              a2 = fma(fd, fd, a2);
              ay = fma((double)s_yf[16 * ks + 8 * lhk + j], fd, ay);
            }
            mfx_split16(fv, x, y);
            bh[j] = x; bl[j] = y;
          }
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afh[ks], bh, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afh[ks], bl, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afl[ks], bh, acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (!XC) {
          a2 += __shfl_xor(a2, 32);
          ay += __shfl_xor(ay, 32);
          const bool act = n < N;
          const double nrm = sqrt(a2);
          const double inv = (act && a2 > 0.0) ? 1.0 / nrm : 0.0;
          const double z = ay * inv;
          const float zf = act ? (float)z : -1e30f, nf = (act && a2 > 0.0) ? (float)nrm : 0.0f;
          // (both halves hold the same values and write them: the FP64 criteria read them back from LDS in every lane)
          s_Zf[NP + n] = zf;
          s_cs[NP + n] = nf;
          double sb = (act && z > 0.0) ? z * z : 0.0;
          int nb = n;
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) {
            const double s2 = __shfl_xor(sb, o);
            const int n2 = __shfl_xor(nb, o);
            const bool take = (s2 > sb) || (s2 == sb && n2 < nb);
            sb = take ? s2 : sb;
            nb = take ? n2 : nb;
          }
          sb = mfx_readlane_f64(sb, 0);
          nb = __builtin_amdgcn_readfirstlane(nb);
          if (lane == 0) {
            const double b2 = *s_bs2;
            if (sb > b2 || (sb == b2 && sb > 0.0 && nb < *s_bn2)) { *s_bs2 = sb; *s_bn2 = nb; }
          }
          // a pair matters only if it beats every single atom: the threshold rises BEFORE the tile is screened
          if (lane == 0 && sb - mrg > 0.0) atomicMax(&s_thr[0], mfx_nonneg_bits(sb - mrg));
          __builtin_amdgcn_wave_barrier();
          sc_thr = s_thr[0];
          sc_z2 = zf;   // the column constants straight from the registers just made
          sc_s = nf;
          scan_main(acc, ct);
        } else {
          scan_tile(acc, ct);
        }
      }
#ifdef MFX_STAMPS_RND
      if (a.stamps && lane == 0) atomicAdd(&a.stamps[(size_t)blockIdx.x * 16 + 12], (unsigned long long)dbg_flagged + ((unsigned long long)dbg_groups << 32));
#endif
      __syncthreads();   // all appends of the round are in the ring, D2's statistics in LDS
      if constexpr (!XC) {
        // D2's best single atom joins the threshold, as after phase 1 (k2s_shared.h)
        k2s_best_single_late<NW>(a, L, tid, mrg);
      }
#ifdef MFX_STAMPS_RND
      if (a.stamps && tid == 0 && round < 4) a.stamps[(size_t)blockIdx.x * 16 + 2 * round + 2] = __builtin_amdgcn_s_memtime();
#endif
      continue;
    }

    // ---- LDS sweep, ping-pong between the two wave groups (waves 0-3 | 4-7: one wave of each per SIMD): while one
    // group runs the 3*KS MFMAs of a column chunk the other one does VALU work (pair screen of its previous
    // accumulator tile + its half of the generation of a coming chunk), so the matrix pipe and the vector ALUs of
    // a SIMD are busy at the same time.  Generation item = (pair of adjacent atoms, the 8 rows of one MFMA
    // fragment); a group owns KS of the 2*KS fragment row blocks of a chunk, one item per thread: gen_load issues
    // its table loads, gen_store converts and writes the FP16 hi/lo fragments.  The two schedules are below.
    const int grp = wave >> 2, tg = tid & 255;
    static_assert(KS <= 16, "one generation item per thread");
    f32x4 gd[8];   // item = (pair of adjacent atoms, the 8 rows of one fragment): 16-byte loads, see phase 1
    const int gq = KS * grp + (tg >> 4);      // fragment row block (k-step, half) = gq; rows 8 gq .. 8 gq + 7
    const bool gact = (tg >> 4) < KS;
    auto gen_load = [&](int ch) {
      const int nn = min(ch * 32 + 2 * (tg & 15), ldn - 2);
      const int q = gact ? gq : KS * grp;     // idle threads repeat a valid address, gen_store skips them
#pragma unroll
      for (int e = 0; e < 8; ++e) gd[e] = tab32x2_at(s_rs[MP + 8 * q + e], nn);
    };
    // the item's interpolation offsets are the same for every chunk of the round: registers, not LDS
    // (not for KS = 16: its A tile takes 128 registers and every further one spills)
#ifndef MFX_XC_GT
#define MFX_XC_GT 0   // (the CSF form needs the registers: with the offsets in registers it spilled 26-29, 11 scratch accesses per period)
#endif
    constexpr bool GT = KS <= 13 && (!XC || MFX_XC_GT);
    float g_t[GT ? 8 : 1];
    if constexpr (GT) {
#pragma unroll
      for (int e = 0; e < 8; ++e) g_t[e] = s_t0f[MP + 8 * (gact ? gq : KS * grp) + e];
    }
    auto gen_store = [&](int ch, int buf) {
      if (gact) {
        const int c0 = 2 * (tg & 15);
        h8 hi0, lo0, hi1, lo1;
        float gu0 = 0.0f, gu1 = 0.0f;   // XC: u2 of the item's two atoms, for the spare row M
        if constexpr (XC) { gu0 = s_uf[NP + ch * 32 + c0]; gu1 = s_uf[NP + ch * 32 + c0 + 1]; }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = GT ? g_t[GT ? e : 0] : s_t0f[MP + 8 * gq + e];
          _Float16 x, y;
          float v0 = fmaf(gd[e][1], t, gd[e][0]), v1 = fmaf(gd[e][3], t, gd[e][2]);
          if constexpr (XC) { if (e == 7) { const bool spare = (gq == 2 * KS - 1); v0 = spare ? gu0 : v0; v1 = spare ? gu1 : v1; } }
          mfx_split16(v0, x, y);
          hi0[e] = x; lo0[e] = y;
          mfx_split16(v1, x, y);
          hi1[e] = x; lo1[e] = y;
        }
        // fragments of atoms c0, c0+1 are adjacent: 32 contiguous bytes per lane, conflict-free
        const int off = (gq * 32 + c0) << 3;
        _Float16* dh = sBh + buf * KS * 512 + off;
        _Float16* dl = sBl + buf * KS * 512 + off;
        *(h8*)dh = hi0; *(h8*)(dh + 8) = hi1;
        *(h8*)dl = lo0; *(h8*)(dl + 8) = lo1;
      }
    };
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    // the 3*KS MFMAs of this wave's row tile against the chunk image in buffer buf
    auto mfma_chunk = [&](int buf) {
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
      const _Float16* bhp = sBh + buf * KS * 512 + lane * 8;
      const _Float16* blp = sBl + buf * KS * 512 + lane * 8;
      h8 bh = *(const h8*)bhp, bl = *(const h8*)blp;
      mfx_static_for<0, KS>([&](auto kc) {
        constexpr int ks = decltype(kc)::value;
        h8 bhn = bh, bln = bl;
        if constexpr (ks + 1 < KS) {   // fragments of the next k-step while this one multiplies
          bhn = *(const h8*)(bhp + (ks + 1) * 512);
          bln = *(const h8*)(blp + (ks + 1) * 512);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afh[ks], bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afh[ks], bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afl[ks], bh, acc, 0, 0, 0);
        bh = bhn; bl = bln;
        __builtin_amdgcn_sched_barrier(0);
      });
    };

    if (round == 0) MFX_STAMP(3);
#ifdef MFX_STAMPS_RND   // diagnostic builds: start and end of every round's sweep (tools/dev_stamps_rnd.py)
    if (a.stamps && tid == 0 && round < 4) a.stamps[(size_t)blockIdx.x * 16 + 2 * round + 1] = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (NB == 3) {
      // ---- one barrier per chunk.  In period c both groups multiply chunk c - group 0 first, group 1 second - and
      // do their VALU work in the other phase: group 0 then screens chunk c and generates its half of chunk c+2,
      // group 1 first screens chunk c-1 and generates its half of chunk c+1.  Chunk c lives in buffer c mod 3:
      // during period c nobody writes it, group 1 writes buffer (c+1) mod 3 (last read in period c-2) and group 0
      // buffer (c+2) mod 3 (last read in period c-1), so the two phases of a period need no barrier between them:
      // a wave moves on to its second phase as soon as its first is done instead of waiting for the slower group
      // (the screening wave has nobody to cover its LDS round trips and in-order table loads: ~2 250 cycles against
      // 1 330 for the MFMA chain when the half-steps were coupled by a barrier).
      // Table loads of a group's next item go at the end of its VALU phase and are consumed one period later.
      gen_load(0);
      gen_store(0, 0);
      if (grp == 0) {
        if (ntiles > 1) { gen_load(1); gen_store(1, 1); }
        if (ntiles > 2) gen_load(2);
      } else if (ntiles > 1) {
        gen_load(1);
      }
      __syncthreads();
      if (round == 0) MFX_STAMP(4);
      thr = __longlong_as_double((long long)s_thr[0]);
      int b0 = 0;   // buffer of chunk c
#ifdef MFX_EXP_NOGEN   // timing experiment (wrong results): rounds after the first find their chunk images ready-made
      const bool exp_gen = round == 0;
#else
      constexpr bool exp_gen = true;
#endif
      for (int c = 0; c <= ntiles; ++c) {
#ifdef MFX_STAMPS_HS   // diagnostic builds: start of 16 periods as seen by wave 0 (tools/dev_stamps_hs.py; default: periods 10..25 of round 1)
#ifndef MFX_HS_ROUND
#define MFX_HS_ROUND 1
#define MFX_HS_C0 10
#endif
        if (a.stamps && round == MFX_HS_ROUND && c >= MFX_HS_C0 && c < MFX_HS_C0 + 16 && tid == 0) a.stamps[(size_t)blockIdx.x * 16 + c - MFX_HS_C0] = __builtin_amdgcn_s_memtime();
#endif
        const int b1 = b0 == 2 ? 0 : b0 + 1, b2 = b1 == 2 ? 0 : b1 + 1;   // buffers of chunks c+1, c+2
        if (grp == 0) {
          if (c < ntiles) {
            if (rt_valid) { mfma_chunk(b0); scan_pre(c); }
            if (exp_gen && c + 2 < ntiles) gen_store(c + 2, b2);
            if (rt_valid) scan_main(acc, c);
            if (exp_gen && c + 3 < ntiles) gen_load(c + 3);
          }
        } else {
          if (c >= 1 && rt_valid) scan_pre(c - 1);
          if (exp_gen && c + 1 < ntiles) gen_store(c + 1, b1);
          if (c >= 1 && rt_valid) scan_main(acc, c - 1);
          if (exp_gen && c + 2 < ntiles) gen_load(c + 2);
          if (c < ntiles && rt_valid) mfma_chunk(b0);
        }
        // LDS-only workgroup barrier: __syncthreads() would also wait for the table loads just issued (vmcnt)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        b0 = b1;
      }
    } else {
      // ---- two chunk images: a barrier after every half-step.  Group g multiplies chunk c in half-step 2c+g and
      // screens it in half-step 2c+g+1; chunk c lives in buffer c&1, read in half-steps 2c, 2c+1 and written in
      // 2c-2 (group 1's half) and 2c-1 (group 0's half), i.e. while buffer (c-1)&1 is being read.  gen_load issues
      // the table loads at the start of the group's MFMA half-step, gen_store converts and writes the FP16 hi/lo
      // fragments in its next VALU half-step (the loads fly behind the MFMAs).
      gen_load(0);
      gen_store(0, 0);
      if (grp == 1 && ntiles > 1) { gen_load(1); gen_store(1, 1); }
      __syncthreads();
      if (round == 0) MFX_STAMP(4);
      thr = __longlong_as_double((long long)s_thr[0]);
      for (int hs = 0; hs <= 2 * ntiles; ++hs) {
        if ((hs & 1) == grp) {
          const int c = (hs - grp) >> 1;
          if (c < ntiles) {
            if (c + 1 + grp < ntiles) gen_load(c + 1 + grp);   // consumed in this group's next half-step
            if (rt_valid) mfma_chunk(c & 1);
          }
        } else {
          const int c = (hs - 1 - grp) >> 1;
          if (c >= 0 && c < ntiles) {
            if (c + 1 + grp < ntiles) gen_store(c + 1 + grp, (c + 1 + grp) & 1);
            if (rt_valid) scan_tile(acc, c);
          }
        }
        __syncthreads();
      }
    }
    if (round == 0) MFX_STAMP(5);
#ifdef MFX_STAMPS_RND
    if (a.stamps && tid == 0 && round < 4) a.stamps[(size_t)blockIdx.x * 16 + 2 * round + 2] = __builtin_amdgcn_s_memtime();
    if (a.stamps && lane == 0 && round < 3) atomicAdd(&a.stamps[(size_t)blockIdx.x * 16 + 9 + round], (unsigned long long)dbg_flagged + ((unsigned long long)dbg_groups << 32));
#endif
