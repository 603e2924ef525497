// What babe_score_eval (score_eval.hip) and babe_sample_bwe (sample.hip) both need of a babe_eval_desc before the first launch: the
// STFT and CQT geometry, and the descriptor's completeness and range checks.
#pragma once
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

// who: the entry point's name, for the message
inline int eval_desc_check(const babe_eval_desc* e, const char* who) {
    BABE_CHECK_ARG(e->unet_plan && e->unet_state && e->cqt_plan && e->rff_freq && e->film_W && e->film_b && e->env_inv && e->tw4096,
                   "%s: incomplete evaluation descriptor", who);
    BABE_CHECK_ARG(e->K >= 1 && e->K <= 8 && e->rff_n > 0 && e->emb_dim[0] == 2 * e->rff_n, "%s: K = %d, rff_n = %d, emb_dim[0] = %d", who,
                   e->K, e->rff_n, e->emb_dim[0]);
    return BABE_OK;
}
