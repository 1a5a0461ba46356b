// The rank-1 pre-pass on one wave's blocks (derivation, constants and why this is a fragment:
// tmfwm_rank1.h): the one text of embed_rank1_kernel<B> (tmfwm_rank1.hip) and
// embed_rank1_ragged_kernel<B> (tmfwm_ragged_pre.hip).  No include guard and no namespace: each
// kernel includes it inside its own braces, after its prologue.  A kept block's pixels are
// stored; a block the pass leaves wrote nothing, and its first lane runs TMF_RANK1_LEFT.
//
// Expected in scope:
//   B, L, R, LD, NW (Geo<B>'s, LD = B + 1), u53 = 2^-53 (double), u24 = 2^-24 (float);
//   a (an EmbedArgs: the frames, or the ragged frame's one-frame view), pos (this lane's StripPos);
//   lane, g = lane / L, q = lane % L, tile = lds + g * B * LD;
//   lds (kRank1LdsFloats<B> floats, __shared__), pix (kRank1PixWords<B> rows of 64 words, __shared__);
//   the macro TMF_RANK1_LEFT: one statement that appends this block to the includer's list.
    const uint8_t *src = a.src + pos.frame * a.frame_stride;
    uint8_t *dst = a.dst + pos.frame * a.frame_stride;

    float x[R][B];
    {
        uint32_t words[R][NW];
        load_block_rows<B>(src, a.W, pos, q, a.aligned, words);
        luma_rows<B>(words, x);
        // the source bytes wait in LDS until the colour phase
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < NW; ++i) pix[r * NW + i][lane] = words[r][i];
    }
    dct2d_rows_layout<B, false>(x, tile, q);  // :192, D in rows layout
    double xd[R][B];  // D in f64 (exact), the f32 copy is dead until M_fast
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < B; ++j) xd[r][j] = (double)x[r][j];

    // squared row norms (this lane's rows), squared column norms and |D|_F^2, in f64
    double rn[R], cn[B], F = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < B; ++j) acc = __builtin_fma(xd[r][j], xd[r][j], acc);
        rn[r] = acc;
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) acc = __builtin_fma(xd[r][j], xd[r][j], acc);
        cn[j] = group_sum<L>(acc);
        F += cn[j];
    }
    const bool zero = F == 0.0;

    // power iteration on D^T D from the column norms
    double v[B];
#pragma unroll
    for (int j = 0; j < B; ++j) v[j] = zero ? (j == 0 ? 1.0 : 0.0) : cn[j];
    double t[R];
#pragma unroll
    for (int it = 0; it < kRank1Iters; ++it) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < B; ++j) acc = __builtin_fma(xd[r][j], v[j], acc);
            t[r] = acc;
        }
        double w[B], nn = 0.0;
#pragma unroll
        for (int j = 0; j < B; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) acc = __builtin_fma(xd[r][j], t[r], acc);
            w[j] = group_sum<L>(acc);
            nn = __builtin_fma(w[j], w[j], nn);
        }
        const bool live = nn > 0.0 && nn < 1e300;
        const double inv = live ? 1.0 / __builtin_sqrt(nn) : 1.0;
#pragma unroll
        for (int j = 0; j < B; ++j) v[j] = live ? w[j] * inv : v[j];
    }
    // a-posteriori (sigma1_certified's margins): rho = |Dv|^2 / |v|^2, r = D^T D v - rho v
    double nv = 0.0, rho_p = 0.0;
#pragma unroll
    for (int j = 0; j < B; ++j) nv = __builtin_fma(v[j], v[j], nv);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < B; ++j) acc = __builtin_fma(xd[r][j], v[j], acc);
        t[r] = acc;
        rho_p = __builtin_fma(acc, acc, rho_p);
    }
    const double tt = group_sum<L>(rho_p), rho = tt / nv;
    double rn2 = 0.0;
#pragma unroll
    for (int j = 0; j < B; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) acc = __builtin_fma(xd[r][j], t[r], acc);
        const double rj = group_sum<L>(acc) - rho * v[j];
        rn2 = __builtin_fma(rj, rj, rn2);
    }
    const double rr0 = __builtin_sqrt(rn2 / nv) * (1.0 + 16.0 * u53) + 256.0 * u53 * F;
    const double rlo = rho * (1.0 - 256.0 * u53), fhi = F * (1.0 + 256.0 * u53);
    const double gap = (rlo + rlo) - fhi;
    const double lhi = (rho + rr0 * rr0 / (gap > 0.0 ? gap : 1.0)) * (1.0 + 256.0 * u53);
    const double s1hi = __builtin_sqrt(lhi) * (1.0 + 512.0 * u53);
    const double s1lo = __builtin_sqrt(rlo) * (1.0 - 512.0 * u53);
    const double s2hi = __builtin_sqrt(fhi - rlo > 0.0 ? fhi - rlo : 0.0) * (1.0 + 512.0 * u53);
    const double g1 = s1lo - s2hi;
    const double theta = rr0 / (gap > 0.0 ? gap : 1.0);
    const double eps_uv = zero ? 0.0 : 1.01 * theta + kRank1PairUnits * u53 * s1hi / (g1 > 0.0 ? g1 : 1.0) + 0x1p-45;
    bool ok = zero || (gap > 0.0 && g1 > 0.0 && eps_uv <= 0x1p-30 && rho == rho);

    // the unit top pair: v / |v|, u = D v / |D v| (this lane's rows)
    const double vinv = zero ? 1.0 : 1.0 / __builtin_sqrt(nv), tinv = zero ? 1.0 : 1.0 / __builtin_sqrt(tt);
    double uu[R];
#pragma unroll
    for (int r = 0; r < R; ++r) uu[r] = zero ? ((q * R + r) == 0 ? 1.0 : 0.0) : t[r] * tinv;
#pragma unroll
    for (int j = 0; j < B; ++j) v[j] = v[j] * vinv;

    // M_fast = f32(D + c u v^T) (:198 + :201 with the top pair alone)
    const uint32_t wv = pos.valid ? a.wm[pos.frame * a.wm_stride + (int64_t)pos.bi * a.nbw + pos.bj] : 0u;
    const double cw = a.alpha * ((double)wv / 255.0);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < B; ++j) x[r][j] = (float)__builtin_fma(cw * uu[r], v[j], xd[r][j]);

    // eps_Y (tools/exp/idct_bound.py): |M_ref - M_fast| <= dM = al a b^T + be u' v'^T + ga 1 1^T and
    // |M_ref|, |M_fast| <= Mb = (1 + al) a b^T + (|c| + be) u' v'^T + ga 1 1^T; the f32 IDCT is
    // IDCT_fl(M) = C' M C'^T + R, |R| <= u (E |M| |C'|^T + |C'| |M| E^T) + u^2 E |M| E^T (C' its exact
    // map, E its first-order rounding bound: IdctBound<B>), so with d_t, m_t the weights above,
    //   eps_Y = sum_t d_t (|C'| x_t)(|C'| y_t)^T + 2 u m_t ((E x_t)(|C'| y_t)^T + (|C'| x_t)(E y_t)^T
    //           + u (E x_t)(E y_t)^T),
    // per pixel (p, q): sum_t A_t(p) P_t(q) + EA_t(p) Q_t(q), P_t = d_t B_t + 2 u m_t EB_t,
    // Q_t = 2 u m_t (B_t + u EB_t), A_t = |C'| x_t, EA_t = E x_t, B_t = |C'| y_t, EB_t = E y_t
    using Tb = IdctBound<B>;
    const float e = (float)eps_uv * (1.0f + 0x1p-20f);
    const float cabs = (float)__builtin_fabs(cw) * (1.0f + 0x1p-20f), s1f = (float)s1hi * (1.0f + 0x1p-20f);
    const float al = 1.01f * (B + 6) * u24, be = 1.01f * ((B + 6) * u24 * cabs + 2.0f * u24 * (s1f + cabs));
    constexpr float resid = (float)(kRank1ResidUnits * u53);  // 2^-40, exact
    const float ga = resid * s1f + cabs * e * (2.0f + e);
    const float w1 = 2.0f * u24 * (1.0f + al), w2 = 2.0f * u24 * (cabs + be);  // 2 u m_1, 2 u m_2
    float ra[R], ru[R];  // a_i = |D_i,:|^(1/2), u'_i = |u_i| + e on this lane's rows
#pragma unroll
    for (int r = 0; r < R; ++r) {
        ra[r] = __builtin_sqrtf(__builtin_sqrtf((float)rn[r] * (1.0f + 0x1p-20f))) * (1.0f + 0x1p-20f);
        ru[r] = (float)__builtin_fabs(uu[r]) + e;
    }
    float av[B], uv[B];  // all rows' a_i and u'_i
    static_for<B>([&](auto K) {
        av[K] = row_value<B, L, K>(ra);
        uv[K] = row_value<B, L, K>(ru);
    });
    float P1[B], Q1[B], P2[B], Q2[B];  // terms a b^T and u' v'^T, every column q
#pragma unroll
    for (int qq = 0; qq < B; ++qq) {
        float sb = 0.0f, eb = 0.0f, sv = 0.0f, ev = 0.0f;
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const float bj = __builtin_sqrtf(__builtin_sqrtf((float)cn[j] * (1.0f + 0x1p-20f))) * (1.0f + 0x1p-20f);
            const float vj = (float)__builtin_fabs(v[j]) + e;
            sb = __builtin_fmaf(Tb::absc[qq][j], bj, sb);
            eb = __builtin_fmaf(Tb::err[qq][j], bj, eb);
            sv = __builtin_fmaf(Tb::absc[qq][j], vj, sv);
            ev = __builtin_fmaf(Tb::err[qq][j], vj, ev);
        }
        P1[qq] = __builtin_fmaf(al, sb, w1 * eb);
        Q1[qq] = w1 * __builtin_fmaf(u24, eb, sb);
        P2[qq] = __builtin_fmaf(be, sv, w2 * ev);
        Q2[qq] = w2 * __builtin_fmaf(u24, ev, sv);
    }

    dct2d_rows_layout<B, true>(x, tile, q);  // :204, Y_fast

    // :207-216 at both ends of [Y_fast - eps_Y, Y_fast + eps_Y]
    bool unc = false, hot = false;  // hot: tmfwm_colour_tail.h
    uint32_t outw[R][NW];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float Ap = 0.0f, EAp = 0.0f, Up = 0.0f, EUp = 0.0f, Sp = 0.0f, ESp = 0.0f;
        // A_t(p), EA_t(p): the tables' row of this pixel row (p = q R + r is lane-dependent: the
        // entries come from the tables by a select over the L lanes' rows)
        static_for<B>([&](auto I) {
            float cpi = Tb::absc[r][I], epi = Tb::err[r][I];
            static_for<L - 1>([&](auto Q1_) {
                constexpr int QQ = Q1_ + 1;
                if (QQ * R + r < B) {
                    cpi = q == QQ ? Tb::absc[(QQ * R + r) % B][I] : cpi;
                    epi = q == QQ ? Tb::err[(QQ * R + r) % B][I] : epi;
                }
            });
            Ap = __builtin_fmaf(cpi, av[I], Ap);
            EAp = __builtin_fmaf(epi, av[I], EAp);
            Up = __builtin_fmaf(cpi, uv[I], Up);
            EUp = __builtin_fmaf(epi, uv[I], EUp);
            Sp += cpi;
            ESp += epi;
        });
        uint32_t words[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) words[i] = pix[r * NW + i][lane];
        // Y's interval of pixel c of this row: [Y_fast - eps_Y, Y_fast + eps_Y]
        const auto yint = [&](int c) {
            const float y = x[r][c];
            // the ones term's column factors are compile-time sums of the tables
            float B3 = 0.0f, EB3 = 0.0f;
#pragma unroll
            for (int j = 0; j < B; ++j) {
                B3 += Tb::absc[c][j];
                EB3 += Tb::err[c][j];
            }
            const float t3 = Sp * __builtin_fmaf(2.0f * u24, EB3, B3) + ESp * (2.0f * u24) * __builtin_fmaf(u24, EB3, B3);
            const float ey = (Ap * P1[c] + EAp * Q1[c] + Up * P2[c] + EUp * Q2[c] + ga * t3) * (1.0f + 0x1p-16f) +
                             __builtin_fabsf(y) * 0x1p-22f + 0x1p-40f;
            return TailY{y - ey, y + ey, 2.0f * ey};
        };
        colour_tail_row<B>(words, yint, outw[r], unc, hot);
    }
    ok = ok && group_or<L>(unc ? 1 : 0) == 0;
    if (!pos.valid) return;
    if (ok) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint8_t *pp = dst + ((int64_t)(pos.bi * B + q * R + r) * a.W + (int64_t)pos.bj * B) * 3;
            if (real_row<B>(q, r)) store_words<B>(pp, a.aligned, outw[r]);
        }
    } else if (q == 0) {
        TMF_RANK1_LEFT
    }
