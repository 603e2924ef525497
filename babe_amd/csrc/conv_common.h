// Pieces shared by the conv translation units (conv*.hip).
//   device: the fused epilogue and sel_scale (conv.hip, conv_bf16.hip; conv11p.hip for the weights' layout), the A-operand fragment
//           read, and conv_w_tap, the one statement of how a packed image reads the reference weight (every pack_* kernel);
//   host:   what the launchers, the *_supported rules and the packed_size / pack_weights entry points have in common: padding,
//           the (co, ci) of the executed op and the weight shapes each kernel family takes, view alignment, the 32-bit offset
//           limits and the time x frequency split of a tile.
#pragma once
#include "common.h"
#include "../../include/babe_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ float sel_scale(bool has, float loaded) { return has ? loaded : 1.f; }

// Tap (kh, kw) between channels (co, ci) of the op a packed image EXECUTES, read from the reference weight w [Cout][Cin][KH][KW]:
// tf 0 the conv itself; tf 1 its input-VJP, the transposed conv: packed Cout = reference Cin, packed Cin = reference Cout, taps
// flipped on both axes.  0 for the padded channels of the image.
__device__ __forceinline__ float conv_w_tap(const float* __restrict__ w, int Cout, int Cin, int KH, int KW, int tf, int co, int ci,
                                            int kh, int kw) {
    if (!tf) return (co < Cout && ci < Cin) ? w[(((long)co * Cin + ci) * KH + kh) * KW + kw] : 0.f;
    return (co < Cin && ci < Cout) ? w[(((long)ci * Cin + co) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)] : 0.f;
}

// Epilogue shared by all conv kernels: out = alpha*acc*oscale[b,co] + rbeta*res; HAS_FB (the (1,1) kernels): acc + fbias[co][f] in
// place of acc.  The 16 loads of a 32x32 tile are
// issued back-to-back inside ONE wave-uniform branch per operand: a per-element "if (ptr) load" makes hipcc branch
// around every load and wait vmcnt(0) each time (measured: the epilogue then serialises 128 load latencies).
template <int NT, int WP, bool HAS_OS, bool HAS_RES, bool HAS_FB = false>
__device__ __forceinline__ void conv_epilogue_impl(const babe_conv_args& a, f32x16 (&acc)[NT][WP], int b, int co0,
                                                   int f0, int t0, int pt_log2, int wave, int l31, int h) {
    const int PT = 1 << pt_log2;
#pragma unroll
    for (int wp = 0; wp < WP; ++wp) {
        const int p = (wave * WP + wp) * 32 + l31;
        const int f = f0 + (p >> pt_log2);
        const int t = t0 + (p & (PT - 1));
        const bool pv = f < a.F && t < a.T;
        const long sp = pv ? (long)f * a.T + t : 0;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float os[16], rr[16], fb[16];
            int cc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                cc[r] = co < a.Cout ? co : a.Cout - 1;
            }
            if constexpr (HAS_OS) {
#pragma unroll
                for (int r = 0; r < 16; ++r) os[r] = a.oscale[b * a.Cout + cc[r]];
            }
            if constexpr (HAS_RES) {
#pragma unroll
                for (int r = 0; r < 16; ++r) rr[r] = a.res[(long)b * a.res_bs + (long)cc[r] * a.res_cs + sp];
            }
            if constexpr (HAS_FB) {
                const int fr = pv ? f : 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) fb[r] = a.fbias[(long)cc[r] * a.F + fr];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                float v = acc[nt][wp][r];
                if constexpr (HAS_FB) v = __fadd_rn(v, fb[r]);
                v *= a.alpha;
                if constexpr (HAS_OS) v *= os[r];
                if constexpr (HAS_RES) v += a.rbeta * rr[r];
                if (pv && co < a.Cout) a.out[(long)b * a.out_bs + (long)co * a.out_cs + sp] = v;
            }
        }
    }
}

template <int NT, int WP>
__device__ __forceinline__ void conv_epilogue(const babe_conv_args& a, f32x16 (&acc)[NT][WP], int b, int co0, int f0,
                                              int t0, int pt_log2, int wave, int l31, int h) {
    // four straight-line specialisations behind wave-uniform branches
    if (a.oscale) {
        if (a.res) conv_epilogue_impl<NT, WP, true, true>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
        else conv_epilogue_impl<NT, WP, true, false>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
    } else {
        if (a.res) conv_epilogue_impl<NT, WP, false, true>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
        else conv_epilogue_impl<NT, WP, false, false>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
    }
}

// the same with the frequency bias a.fbias (non-NULL); instantiated by the (1,1) kernels only
template <int NT, int WP>
__device__ __forceinline__ void conv_epilogue_fb(const babe_conv_args& a, f32x16 (&acc)[NT][WP], int b, int co0, int f0,
                                                 int t0, int pt_log2, int wave, int l31, int h) {
    if (a.oscale) {
        if (a.res) conv_epilogue_impl<NT, WP, true, true, true>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
        else conv_epilogue_impl<NT, WP, true, false, true>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
    } else {
        if (a.res) conv_epilogue_impl<NT, WP, false, true, true>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
        else conv_epilogue_impl<NT, WP, false, false, true>(a, acc, b, co0, f0, t0, pt_log2, wave, l31, h);
    }
}

template <int N> struct AVec;
template <> struct AVec<1> { static __device__ __forceinline__ void ld(const float* p, float* v) { v[0] = p[0]; } };
template <> struct AVec<2> {
    static __device__ __forceinline__ void ld(const float* p, float* v) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = t.x; v[1] = t.y;
    }
};
template <> struct AVec<3> {
    static __device__ __forceinline__ void ld(const float* p, float* v) { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; }
};
template <> struct AVec<4> {
    static __device__ __forceinline__ void ld(const float* p, float* v) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
};

// ---- host scaffolding

inline int pad_to(int x, int m) { return (x + m - 1) / m * m; }

inline int ilog2_floor(int v) {
    int l = 0;
    while ((1 << (l + 1)) <= v) ++l;
    return l;
}
inline int ilog2_ceil(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// 32-row output-channel tiles per workgroup of the direct kernels: the largest of 4..1 that divides the tile count
inline int pick_nt(int CoutP) {
    const int n32 = CoutP / 32;
    for (int c = 4; c >= 1; --c)
        if (n32 % c == 0) return c;
    return 1;
}

// (output, input) channels of the op a packed image executes (conv_w_tap): swapped under transpose_flip
struct ConvIO {
    int co, ci;
};
inline ConvIO conv_exec_io(int Cout, int Cin, int transpose_flip) {
    return transpose_flip ? ConvIO{Cin, Cout} : ConvIO{Cout, Cin};
}

// Which weight shapes a kernel family takes, on the (ci, co) of the EXECUTED op: the channel clauses of that family's *_supported
// rule and, through babe_packed_conv_plan (conv_auto.hip), the reason a direction has the family's image.  Stated here only.
//   nested F(2,5) x F(4,3): no padded input channels and an even number of 8-channel slabs (the channel part of a load address is
//   a scalar offset the buffer range check does not cover; the slab loop is unrolled by two), more than one 32-channel tile out
inline bool conv_wino45_shape(int ci, int co, int KH, int KW) { return KH == 5 && KW == 3 && ci >= 16 && ci % 16 == 0 && co > 32; }
//   nested F(4,5) x F(4,3): the same input rule, output channels a whole number of 128-, 96- or 64-channel tiles
inline bool conv_wino85_shape(int ci, int co, int KH, int KW) {
    return KH == 5 && KW == 3 && ci >= 16 && ci % 16 == 0 && (co % 128 == 0 || co % 96 == 0 || co % 64 == 0);
}
//   few-output-channel vector kernel, which reads the RAW weights: 3 taps along time, at most 4 output channels
inline bool conv_fewco_shape(int co, int KW) { return KW == 3 && co >= 1 && co <= 4; }

// a [B][C][F][T] float view whose rows may be read / written as `bytes`-wide vectors (16: float4, 8: float2)
inline bool view_aligned(const void* p, long bs, long cs, int bytes = 16) {
    return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0 && bs % (bytes / 4) == 0 && cs % (bytes / 4) == 0;
}

// Limits of what one buffer descriptor (or a kernel's own 32-bit offset arithmetic) may span: floats below 2 GiB, floats below
// 1 GiB (the nested Winograd kernels, whose out-of-range marker is bit 30), bytes below 2 GiB.
constexpr long LIM_F32_2G = 0x7fffffffL / 4, LIM_F32_1G = 0x3fffffffL / 4, LIM_BYTES_2G = 0x7fffffffL;
inline bool fits_i32(long n, long lim = LIM_F32_2G) { return n < lim; }

// Geometry argument of the kernels that tile (frequency rows x time) into power-of-two tiles.  Kernels with more fields keep a
// struct of their own (ConvGeomB, Bf16pGeom, Wino45Geom, Wino85Geom).
struct ConvTileGeom {
    int CinP, CoutP, pt_log2, pr_log2, tiles_t;
};

// A tile of 2^npos_log2 positions as 2^pr_log2 rows x 2^pt_log2 time steps: the power of two that covers T, at most the whole
// tile and at least 2^min_pt_log2.  CinP / CoutP are the 8 / 32 padding of the packed images; *tiles_f = row tiles.
inline ConvTileGeom conv_tile_geom(const babe_conv_args& a, int npos_log2, int min_pt_log2, int* tiles_f) {
    ConvTileGeom g;
    g.CinP = pad_to(a.Cin, 8);
    g.CoutP = pad_to(a.Cout, 32);
    g.pt_log2 = ilog2_ceil(a.T);
    if (g.pt_log2 > npos_log2) g.pt_log2 = npos_log2;
    if (g.pt_log2 < min_pt_log2) g.pt_log2 = min_pt_log2;
    g.pr_log2 = npos_log2 - g.pt_log2;
    g.tiles_t = cdiv(a.T, 1 << g.pt_log2);
    *tiles_f = cdiv(a.F, 1 << g.pr_log2);
    return g;
}

}  // namespace
