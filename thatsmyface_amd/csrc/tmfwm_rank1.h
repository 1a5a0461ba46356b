// The rank-1 pre-pass of the hybrid route (TMFWM_ROUTE_RANK1, round 6), photo mode,
// what its two kernels share.
//
// The reference reconstructs every block from all of LAPACK's factors rounded to f32
// (watermarking.py:195-201), but only S[0] changes, so its M_ref = fl(U32 fl(S'32 Vt32)) is
// D + c u1 v1^T up to rounding (c = alpha w / 255).  This pass computes, per block, the top
// singular pair (u, v) by an f64 power iteration with an a-posteriori bound, M_fast =
// f32(D + c u v^T), Y_fast = IDCT_fl(M_fast), and a per-pixel bound eps_Y >= |Y_ref - Y_fast|:
//   dM_ij <= alpha' G_ij + beta' P_ij + gamma'      (tools/exp/fastpath_study.py, round 4)
//     G_ij = |D_i,:|^(1/2) |D_:,j|^(1/2) bounds sum_t |U_it| s_t |V_jt| (Cauchy-Schwarz: the rows of
//       U and V are unit vectors), P_ij = (|u_i| + e)(|v_j| + e) bounds |u1_i| |v1_j| of LAPACK's top
//       pair (e = eps_uv, below), alpha' = 1.01 (b + 6) 2^-24 (the b fmaf roundings of the chain,
//       the 4 factor roundings, f32(M_fast)), beta' = 1.01 ((b + 6) 2^-24 |c| + 2^-23 (s1 + |c|))
//       (S[0]'s and S'[0]'s f32 roundings), gamma' = 2^-40 s1 (LAPACK's residual |U S V^T - D|,
//       8192 units of 2^-53 s1, 84 times the worst measured) + |c| e (2 + e);
//   eps_Y = |C'| dM |C'|^T + 2 (u (E Mb |C'|^T + |C'| Mb E^T) + u^2 E Mb E^T),  Mb = G + |c| P + dM
//     bounding both |M_ref| and |M_fast|; C' the f32 IDCT's exact linear map, E the first-order
//     bound of its roundings per input (|IDCT_fl(x) - C' x| <= u E |x|), both from a transcription
//     of the op sequence (tools/exp/idct_bound.py -> tmfwm_idct_bounds.h, every slider length) --
//     rank-three, so per pixel six products of |C'|- and E-transformed vectors;
// and keeps a block's bytes when every channel gives the same byte at Y_fast - eps_Y and
// Y_fast + eps_Y (each channel is monotone in Y).  Top pair: with v the iterate, rho = |Dv|^2 /
// |v|^2, r = D^T D v - rho v and F = |D|_F^2, the extract's Kato-Temple margins (sigma1_certified)
// give lambda_1 in [rho, rho + |r|^2 / gap], gap = 2 rho - F, and Davis-Kahan sin(v, v1) <=
// |r| / (|v| gap); u = D v / |D v| is no further from u1; LAPACK's own top pair is within
// 1024 2^-53 s1 / (s1 - s2) (6.4 times the worst measured, tools/exp/lapack_bounds.py; the
// pass requires e <= 2^-30, so e's share of the bound is below 2^-29 |c| whatever that constant).
// A block that fails any test (no spectral gap, an undecided byte) writes nothing and goes to the
// slow list, whose list pass (embed_kernel<b, true>) redoes it on the full hybrid route -- Jacobi
// SVD, byte certificate, dgesdd route (TMFWM_ROUTE_RANK1) -- or straight to the dgesdd route
// (TMFWM_ROUTE_RANK1_REFERENCE, no Jacobi factors and so no K), so every byte is the reference's
// either way.
//
// This header is the pass's constants and helpers; its statements are tmfwm_rank1_body.h, a
// fragment that embed_rank1_kernel<B> (tmfwm_rank1.hip) and embed_rank1_ragged_kernel<B>
// (tmfwm_ragged_pre.hip) each include inside their own braces, between a prologue (LDS, position)
// and TMF_RANK1_LEFT, which says where a block the pass leaves is appended.  A fragment and not a
// device function: with both kernels calling one __forceinline__ function the single-size kernel's
// register allocation moved (VGPRs at b = 6 / 10 / 12 / 14 / 16: 109 / 189 / 184 / 200 / 225 ->
// 111 / 191 / 185 / 222 / 223; SGPRs at b = 8 .. 16: 53 / 61 / 61 / 67 / 67 -> 60 / 70 / 69 / 74 /
// 75), with a, pos and the LDS arrays passed by reference or declared inside it alike.  Included,
// the body compiles in the single-size kernel to the instructions it had written out there, and
// the ragged kernel takes its sibling's VGPR count (profiles/one_body/).  The append is a macro
// because a lambda called at that point, with equal registers, changed the instruction stream.
#pragma once
#include "tmfwm_blocks.h"
#include "tmfwm_idct_bounds.h"

namespace tmf {

template <int B>
constexpr int kRank1Waves = B <= 8 ? 3 : 2;  // waves per SIMD of the pre-pass kernels
// LDS of a pre-pass wave: the transpose tiles, and the source bytes until the colour phase
template <int B>
constexpr int kRank1LdsFloats = Geo<B>::BPW * B * (B + 1);
template <int B>
constexpr int kRank1PixWords = Geo<B>::R * Geo<B>::NW;

constexpr int kRank1Iters = 4;  // f64 power steps before the a-posteriori test
// LAPACK's two measured constants (tools/exp/lapack_bounds.py, profiles/r06/lapack_bounds_b*.json;
// tests/test_rank1_bound.py holds them to tests/k_corpus.py's), in units of 2^-53 sigma_1:
constexpr double kRank1ResidUnits = 8192.0;  // residual |U S V^T - D| per element: gamma' = 2^-40 s1
constexpr double kRank1PairUnits = 1024.0;   // top pair, per element, over (s1 - s2)

// value of element k (0 <= k < B) of a per-row quantity held as R rows per lane (lane k / R)
template <int B, int L, int K>
TMF_DEVI float row_value(const float (&own)[kRows<B, L>])
{
    constexpr int R = kRows<B, L>;
    return group_bcast<L, K / R>(own[K % R]);
}

}  // namespace tmf
