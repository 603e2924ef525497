// What babe_score_eval (score_eval.hip), babe_sample_bwe (sample.hip) and babe_restore_recording (recording.hip) need of a
// babe_eval_desc and of a step table before the first launch: the STFT and CQT geometry, and the completeness and range checks.
#pragma once
#include <cmath>
#include "common.h"
#include "../../include/babe_hip.h"

struct EvalGeom {
    int hop, frames, nbins;           // STFT
    int nocts, binsoct, T_oct[8];     // CQT
};

inline bool eval_dims_ok(const babe_eval_desc* e) { return e->nfft >= 256 && e->L >= e->nfft; }

// false: the CQT plan is missing or has no design.  The STFT fields need no plan and are filled either way.
inline bool geom(const babe_eval_desc* e, EvalGeom& g) {
    g.hop = e->nfft / 2;
    g.frames = 1 + e->L / g.hop;
    g.nbins = g.hop + 1;
    const void* d = babe_cqt_plan_design(e->cqt_plan);
    if (!d) return false;
    long nb = 0;
    babe_cqt_design_get(d, "nb", &nb, 8);
    const long bytes = babe_cqt_design_get(d, "T_oct", nullptr, 0);
    if (bytes <= 0 || bytes > 32) return false;
    babe_cqt_design_get(d, "T_oct", g.T_oct, 32);
    g.nocts = (int)(bytes / 4);
    g.binsoct = (int)(nb / g.nocts);
    return true;
}

// the evaluation reads params / specY only through the STFT filter
inline bool eval_reads_params(const babe_eval_desc* e, bool has_y) { return has_y && e->obs_kind == BABE_OBS_STFT; }

// the known observation model (obs_kind and its parameters, dc_classic, y == NULL), host only
inline int eval_obs_check(const babe_eval_desc* e, bool has_y, const char* who) {
    const int k = e->obs_kind;
    BABE_CHECK_ARG(k >= BABE_OBS_STFT && k <= BABE_OBS_CLIP, "%s: bad descriptor: obs_kind = %d is no BABE_OBS_* value", who, k);
    BABE_CHECK_ARG(k != BABE_OBS_FIR || (e->taps && e->ntaps >= 1), "%s: bad descriptor: BABE_OBS_FIR with NULL taps or ntaps = %d", who,
                   e->ntaps);
    BABE_CHECK_ARG(k != BABE_OBS_IIR || (e->order >= 1 && e->order <= 16), "%s: bad descriptor: BABE_OBS_IIR with order = %d outside 1..16",
                   who, e->order);
    BABE_CHECK_ARG(k != BABE_OBS_IIR || (e->b && e->a), "%s: bad descriptor: BABE_OBS_IIR with NULL b or a", who);
    BABE_CHECK_ARG(k != BABE_OBS_MASK || e->obs_mask, "%s: bad descriptor: BABE_OBS_MASK with NULL obs_mask", who);
    BABE_CHECK_ARG(k != BABE_OBS_MASK || e->obs_mask_bs == 0 || e->obs_mask_bs >= e->L,
                   "%s: bad descriptor: obs_mask_bs = %ld (0, or at least L = %d)", who, e->obs_mask_bs, e->L);
    BABE_CHECK_ARG(k != BABE_OBS_CLIP || e->clip_value >= 0.f, "%s: bad descriptor: BABE_OBS_CLIP with clip_value = %g (must be >= 0)", who,
                   e->clip_value);
    BABE_CHECK_ARG(!(e->dc_classic && k == BABE_OBS_CLIP), "%s: bad descriptor: dc_classic with BABE_OBS_CLIP (the replacement step "
                   "holds for linear A only)", who);
    BABE_CHECK_ARG(!(e->dc_classic && e->dc_mask), "%s: bad descriptor: dc_classic with dc_mask (one replacement step)", who);
    BABE_CHECK_ARG(!(e->blind && k != BABE_OBS_STFT), "%s: bad descriptor: blind = 1 with obs_kind = %d (only the STFT filter is fitted)",
                   who, k);
    BABE_CHECK_ARG(!e->mask || k == BABE_OBS_STFT || k == BABE_OBS_FIR, "%s: bad descriptor: mask with obs_kind = %d (the AR mix goes "
                   "over the STFT filter or a FIR)", who, k);
    BABE_CHECK_ARG(has_y || (k == BABE_OBS_STFT && !e->mask && !e->dc_classic),
                   "%s: bad descriptor: y == NULL (unconditional) with obs_kind = %d, mask or dc_classic", who, k);
    return BABE_OK;
}

// who: the entry point's name, for the message; has_y: the call has observations (false: unconditional)
inline int eval_desc_check(const babe_eval_desc* e, const char* who, bool has_y = true) {
    BABE_TRY(eval_obs_check(e, has_y, who));
    BABE_CHECK_ARG(!(e->mask && e->blind), "%s: mask with blind = 1 (the AR observation model takes a known filter)", who);
    BABE_CHECK_ARG(e->mask || (!e->dc_mask && !e->dc_y), "%s: dc_mask / dc_y without mask", who);
    BABE_CHECK_ARG(!e->dc_mask == !e->dc_y, "%s: dc_mask and dc_y come together", who);
    BABE_CHECK_ARG(!e->mask || e->mask_bs == 0 || e->mask_bs >= e->L, "%s: mask_bs = %ld (0, or at least L = %d)", who, e->mask_bs, e->L);
    BABE_CHECK_ARG(e->unet_plan && e->unet_state && e->cqt_plan && e->rff_freq && e->film_W && e->film_b && e->env_inv && e->tw4096,
                   "%s: incomplete evaluation descriptor", who);
    BABE_CHECK_ARG(e->K >= 1 && e->K <= 8 && e->rff_n > 0 && e->emb_dim[0] == 2 * e->rff_n, "%s: K = %d, rff_n = %d, emb_dim[0] = %d", who,
                   e->K, e->rff_n, e->emb_dim[0]);
    return BABE_OK;
}

// the T rows of a run and its t0 (host memory)
inline int sample_steps_check(const babe_sample_step* steps, int T, float t0, const char* who) {
    BABE_CHECK_ARG(std::isfinite(t0), "%s: t0 is not finite", who);
    for (int i = 0; i < T; ++i) {
        const babe_sample_step& s = steps[i];
        BABE_CHECK_ARG(s.t_hat > 0.f && std::isfinite(s.t_hat) && std::isfinite(s.inject) && std::isfinite(s.h) &&
                           (s.heun == 0 || (s.heun == 1 && s.t_next > 0.f && std::isfinite(s.t_next))),
                       "%s: step %d: t_hat = %g, inject = %g, t_next = %g, h = %g, heun = %d", who, i, s.t_hat, s.inject, s.t_next, s.h, s.heun);
    }
    return BABE_OK;
}
