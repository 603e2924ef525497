// The k = (1,1) ResnetBlocks of the UNet (networks/cqtdiff+.py ResnetBlock :452-493 with one (1,1) dilation layer: the init blocks
// 2 -> N of every octave and the output heads N -> 2, up_out / mid_out) forward as ONE pass over the block's N-channel tensor.
// Everything in such a block is pointwise in (f, t) except the GroupNorm group sums, which babe_gn_partial has formed:
//   scale[c] = gamma[c] (film[c] + 1) / (std_g + eps)                   (csrc/norm.hip; the finalize runs in this pass's prologue)
//   y        = RS2 gate (H gelu(scale z)) + RS2 z                       the dilation layer, H an N x N matrix on fp32 MFMA
//   head:  out = RS2 res_conv(z) + RS2 proj_out(y)   [2 channels]       optionally out = RS2 (that) + RS2 add  (the decoder's Xout)
//   init:  out = RS2 res_conv(x) + RS2 y             [N channels]       z = proj_in(x) from the caller, x the 2-channel block input
// run layer by layer these are five launches that read and write N-channel planes 8 (head) or 8 + 1 (init) times; here z is read
// once and, for the init block, out written once.
//
// A wave owns 32 positions and ALL N channels of them; a workgroup is 4 waves = 128 consecutive positions of the dense (f, t) plane.
//   * z is loaded straight into registers, N/2 values per lane, every load issued before anything waits.  The K index of MFMA step s
//     of half-wave h is channel chan(s, h) = 8 (s / 4) + 4 h + s % 4: with that labelling a lane holds z for exactly the channels
//     whose accumulator rows it will hold (v_mfma_f32_32x32x2_f32: row 8 (r / 4) + 4 h + r % 4 of tile nt is register r, so
//     s = 16 nt + r), and the residual RS2 z needs no second read and no LDS.
//   * gelu(scale z) is formed in registers, as the B operand of the MFMA of its K-step.
//   * H streams through LDS in slabs of 16 input channels (global -> registers one slab ahead -> LDS, two buffers, one barrier per
//     slab), un-permuted from the packed image's in-tile column order into [k][position-in-tile l * NT + nt], so that a lane reads
//     the A operands of all NT row tiles as one contiguous run.  The whole matrix is at most 256 KB and L2-resident.
//   * The tail runs on the accumulators: the N -> 2 projections are per-lane sums in channel order plus one exchange between the
//     two half-waves - a fixed order, no atomics, so both UNet sequencers get the same bits whatever the scheduling.
#include "common.h"
#include "../../include/babe_hip.h"
#include "prof.h"
#include "conv_common.h"
#include "gelu.h"
#include "gn_stat.h"
#include <atomic>
#include <cstdlib>

namespace {

using babe_gelu::gelu_f;

constexpr float PW_RS2 = 0.70710678118654752440f;
constexpr int PW_G = 8;                  // GroupNorm groups (one half-wave of the 256 threads finalises each)
constexpr float PW_EPS = 1e-7f;
constexpr int PW_KC = 16;                // input channels per slab of H
constexpr int PW_POS = 128;              // positions per workgroup

struct PwDev {
    const float* z; long z_bs;           // dense [B][N][FT]
    const float* x; long x_bs, x_cs;     // init: [B][2][FT] view
    float* out; long out_bs, out_cs;
    const float* add; long add_bs, add_cs;
    const double* part;
    const float *gamma, *film, *gate;    // film: the affine vector of item 0; gate [B][N]
    long film_bs;
    float *stats, *scale;
    const float *wH, *wres, *wpo;        // fwd images: H [N][N], res_conv (head [N][32], init [8][N]), proj_out [N][32]
    int ntH, ntres;                      // row tiles the H / res_conv images were packed for
    int FT, S;
    long n;                              // elements of a GroupNorm group
};

// stored column of a packed (1,1) image -> logical output channel (conv.hip pack_weights_kernel)
__device__ __forceinline__ int pw_unperm(int cs, int nt) {
    const int BN = nt * 32, loc = cs % BN;
    return cs - loc + (loc % nt) * 32 + loc / nt;
}

template <int NT>
__device__ __forceinline__ void pw_ld_a(const float* p, float (&v)[NT]) {
    if constexpr (NT % 4 == 0) {
#pragma unroll
        for (int i = 0; i < NT / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else if constexpr (NT % 2 == 0) {
#pragma unroll
        for (int i = 0; i < NT / 2; ++i) {
            const float2 t = reinterpret_cast<const float2*>(p)[i];
            v[2 * i] = t.x; v[2 * i + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NT; ++i) v[i] = p[i];
    }
}

// grid: (ceil(FT / 128), 1, B).  Workgroups per CU the register budget is set for: 4 at N = 64 (3 for the init block, which spills at 4),
// where the planes are largest and the pass has least arithmetic per byte to hide its loads behind, 2 up to N = 128, 1 above (N/2
// values of z + N/2 accumulators)
template <int NT, bool HEAD>
__global__ __launch_bounds__(256, NT <= 2 ? (HEAD ? 4 : 3) : NT <= 4 ? 2 : 1) void pw_fwd_kernel(PwDev a) {
#if __HIP_DEVICE_COMPILE__
    constexpr int N = NT * 32;
    constexpr int NS = N / 2;                         // MFMA K-steps = z values per lane
    constexpr int NSLAB = N / PW_KC;
    constexpr int WJ = PW_KC * N / 256;               // floats of a slab per thread (2 NT)
    __shared__ __attribute__((aligned(16))) float w_sh[2][PW_KC * N];
    __shared__ __attribute__((aligned(16))) float4 t_sh[N];      // head: (res_conv 0, 1, proj_out 0, 1)[c]; init: (res_conv[c][0], [c][1], -, -)
    __shared__ float sc_sh[N], gt_sh[N], r_sh[PW_G];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const long p_raw = (long)blockIdx.x * PW_POS + wave * 32 + l31;
    const bool valid = p_raw < a.FT;
    const long p = valid ? p_raw : a.FT - 1;          // (padding lanes read the last position and store nothing)

    // ---- every load of the pass is issued here, the small L2-resident ones first: vector loads return in order, so the finalize
    // below waits for the partial sums and per-channel operands only and the N/2 loads of z stay in flight behind them
    const int g = tid >> 5, sub = tid & 31;          // GroupNorm finalize: one half-wave per group (gn_finalize_kernel's arithmetic)
    double s0, s1;
    gn_part_sum32(a.part, (long)(b * PW_G + g) * a.S, a.S, sub, s0, s1);
    const int cc = tid < N ? tid : N - 1;             // this thread's channel of the per-channel operands
    const float gam = a.gamma[cc], flm = a.film[(long)b * a.film_bs + cc], gte = a.gate[b * N + cc];
    float4 tw;
    int tdst = cc;
    if constexpr (HEAD) {
        tw = float4{a.wres[cc * 32], a.wres[cc * 32 + 1], a.wpo[cc * 32], a.wpo[cc * 32 + 1]};
    } else {
        tw = float4{a.wres[cc], a.wres[N + cc], 0.f, 0.f};
        tdst = pw_unperm(cc, a.ntres);                // stored column cc of the [8][N] image holds channel tdst
    }
    int woff[WJ];                                     // LDS offset of this thread's j-th float of a slab of H
    float wreg[WJ];
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int idx = tid + j * 256;
        const int k = idx / N, co = pw_unperm(idx % N, a.ntH);
        woff[j] = k * N + (co & 31) * NT + (co >> 5);
        wreg[j] = a.wH[idx];
    }
    float x0 = 0.f, x1 = 0.f;
    if constexpr (HEAD) {
        if (a.add) {
            x0 = a.add[(long)b * a.add_bs + p];
            x1 = a.add[(long)b * a.add_bs + a.add_cs + p];
        }
    } else {
        x0 = a.x[(long)b * a.x_bs + p];
        x1 = a.x[(long)b * a.x_bs + a.x_cs + p];
    }
    float zr[NS];
    {
        const float* zp = a.z + (long)b * a.z_bs + p;
#pragma unroll
        for (int s = 0; s < NS; ++s) zr[s] = zp[(long)((s >> 2) * 8 + 4 * h + (s & 3)) * a.FT];
    }

    // ---- statistics, scales, gates, the tail's weights and slab 0 of H into LDS
    if (sub == 0) {
        const GnStat st = gn_stat(s0, s1, a.n, PW_EPS);
        r_sh[g] = st.r;
        if (blockIdx.x == 0) gn_stat_store(a.stats, b * PW_G + g, st);
    }
    __syncthreads();
    if (tid < N) {
        const float sc = gam * (flm + 1.f) * r_sh[tid / (N / PW_G)];
        sc_sh[tid] = sc;
        if (blockIdx.x == 0) a.scale[b * N + tid] = sc;
        gt_sh[tid] = gte * PW_RS2;
        t_sh[tdst] = tw;
    }
#pragma unroll
    for (int j = 0; j < WJ; ++j) w_sh[0][woff[j]] = wreg[j];
    __syncthreads();

    // ---- acc += H[:, chan(s, h)] gelu(scale z), two K indices per MFMA
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

#pragma unroll
    for (int q = 0; q < NSLAB; ++q) {
        if (q + 1 < NSLAB) {
#pragma unroll
            for (int j = 0; j < WJ; ++j) wreg[j] = a.wH[(q + 1) * PW_KC * N + tid + j * 256];
        }
        const float* Ws = w_sh[q & 1];
#pragma unroll
        for (int sl = 0; sl < PW_KC / 2; ++sl) {
            const int s = q * (PW_KC / 2) + sl;
            const int cl = (sl >> 2) * 8 + 4 * h + (sl & 3);          // channel within the slab
            const float av = gelu_f(zr[s] * sc_sh[q * PW_KC + cl]);
            float wv[NT];
            pw_ld_a<NT>(Ws + cl * N + l31 * NT, wv);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[nt], av, acc[nt], 0, 0, 0);
        }
        if (q + 1 < NSLAB) {
#pragma unroll
            for (int j = 0; j < WJ; ++j) w_sh[(q + 1) & 1][woff[j]] = wreg[j];
            __syncthreads();
        }
    }

    // ---- tail on the accumulators: register r of tile nt is channel 32 nt + 8 (r / 4) + 4 h + r % 4 = chan(16 nt + r, h)
    if constexpr (HEAD) {
        float pr0 = 0.f, pr1 = 0.f, pp0 = 0.f, pp1 = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = nt * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                const float zv = zr[16 * nt + r];
                const float y = __builtin_fmaf(PW_RS2, zv, __fmul_rn(acc[nt][r], gt_sh[c]));
                const float4 w = t_sh[c];
                pr0 = __builtin_fmaf(w.x, zv, pr0);
                pr1 = __builtin_fmaf(w.y, zv, pr1);
                pp0 = __builtin_fmaf(w.z, y, pp0);
                pp1 = __builtin_fmaf(w.w, y, pp1);
            }
        pr0 = __fadd_rn(pr0, __shfl_xor(pr0, 32, 64));
        pr1 = __fadd_rn(pr1, __shfl_xor(pr1, 32, 64));
        pp0 = __fadd_rn(pp0, __shfl_xor(pp0, 32, 64));
        pp1 = __fadd_rn(pp1, __shfl_xor(pp1, 32, 64));
        float o0 = __builtin_fmaf(PW_RS2, pp0, __fmul_rn(pr0, PW_RS2));
        float o1 = __builtin_fmaf(PW_RS2, pp1, __fmul_rn(pr1, PW_RS2));
        if (a.add) {
            o0 = __builtin_fmaf(PW_RS2, x0, __fmul_rn(o0, PW_RS2));
            o1 = __builtin_fmaf(PW_RS2, x1, __fmul_rn(o1, PW_RS2));
        }
        if (valid && h == 0) {
            a.out[(long)b * a.out_bs + p] = o0;
            a.out[(long)b * a.out_bs + a.out_cs + p] = o1;
        }
    } else {
        float* op = a.out + (long)b * a.out_bs + p;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = nt * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                const float y = __builtin_fmaf(PW_RS2, zr[16 * nt + r], __fmul_rn(acc[nt][r], gt_sh[c]));
                const float4 w = t_sh[c];
                const float rc = __builtin_fmaf(w.y, x1, __fmul_rn(w.x, x0));
                const float v = __builtin_fmaf(PW_RS2, y, __fmul_rn(rc, PW_RS2));
                if (valid) op[(long)c * a.out_cs] = v;
            }
    }
#endif
}

template <int NT>
void pw_launch(bool head, const PwDev& d, int B, hipStream_t s) {
    const dim3 grid(cdiv(d.FT, PW_POS), 1, B);
    if (head) hipLaunchKernelGGL((pw_fwd_kernel<NT, true>), grid, dim3(256), 0, s, d);
    else hipLaunchKernelGGL((pw_fwd_kernel<NT, false>), grid, dim3(256), 0, s, d);
}

// BABE_PW_BLOCK: the process's switch, read here and nowhere else
std::atomic<int>& pw_switch() {
    static std::atomic<int> on{[] { const char* e = getenv("BABE_PW_BLOCK"); return e ? (atoi(e) != 0 ? 1 : 0) : 1; }()};
    return on;
}

bool pw_al16(const void* p, long bs, long cs) { return view_aligned(p, bs, cs); }

// row tiles a (1,1) fwd image with co output channels was packed for: the descriptor's nt, 0 = the library default (conv.hip)
int pw_image_nt(const babe_packed_conv& c, int co) { return c.nt > 0 ? c.nt : pick_nt(pad_to(co, 32)); }

// 1 head (N -> 2: up_out, mid_out), 2 init (2 -> N), 0 neither: the block's static shape
int pw_kind(const babe_unet_block& k) {
    const int N = k.N;
    if (k.nd != 1 || k.k53 || N % 32 != 0 || N < 64 || N > 256) return 0;
    const babe_packed_conv& H = k.H[0];
    if (H.KH != 1 || H.KW != 1 || H.Cin != N || H.Cout != N || H.splits != 0 || !H.fwd || H.nt < 0 || (N / 32) % pw_image_nt(H, N) != 0) return 0;
    if (k.fb_proj_in || k.fb_res_conv || !k.gamma[0]) return 0;
    auto c11 = [](const babe_packed_conv& c, int co, int ci) {
        return c.Cout == co && c.Cin == ci && c.KH == 1 && c.KW == 1 && c.splits == 0 && c.fwd && c.nt >= 0 && ((co + 31) / 32) % pw_image_nt(c, co) == 0;
    };
    if (!k.proj_in.Cout && c11(k.proj_out, 2, N) && c11(k.res_conv, 2, N)) return 1;
    if (!k.proj_out.Cout && c11(k.proj_in, N, 2) && c11(k.res_conv, N, 2)) return 2;
    return 0;
}

}  // namespace

extern "C" int babe_pw_block_enable(int on) { return pw_switch().exchange(on ? 1 : 0, std::memory_order_relaxed); }

extern "C" int babe_pw_block_supported(const babe_unet_block* blk, const babe_pw_args* a, int train) {
    if (!blk || !a || train || a->plan_splits != 0 || !pw_switch().load(std::memory_order_relaxed)) return 0;
    const int kind = pw_kind(*blk);
    if (!kind) return 0;
    const int N = blk->N;
    const long FT = (long)a->F * a->T;
    if (a->B < 1 || a->F < 1 || a->T < 4 || a->T % 4 != 0 || a->S < 1) return 0;
    if (!fits_i32((long)N * FT)) return 0;
    if (!a->z || a->z_cs != FT || a->z_bs != (long)N * FT || !pw_al16(a->z, a->z_bs, a->z_cs)) return 0;       // z dense
    if (!a->out || !pw_al16(a->out, a->out_bs, a->out_cs)) return 0;
    if (!a->part || !a->film || !a->gate || !a->stats || !a->scale) return 0;
    if (kind == 1) {
        if (a->x) return 0;
        if (a->add && !pw_al16(a->add, a->add_bs, a->add_cs)) return 0;
    } else {
        if (!a->x || a->add || !pw_al16(a->x, a->x_bs, a->x_cs)) return 0;
    }
    return kind;
}

extern "C" int babe_pw_block_fwd(const babe_unet_block* blk, const babe_pw_args* a, void* stream) {
    const int kind = babe_pw_block_supported(blk, a, 0);
    BABE_CHECK_ARG(kind, "pw_block_fwd: not a block babe_pw_block_supported takes (or the switch is off)");
    const int N = blk->N;
    PwDev d;
    d.z = a->z; d.z_bs = a->z_bs;
    d.x = a->x; d.x_bs = a->x_bs; d.x_cs = a->x_cs;
    d.out = a->out; d.out_bs = a->out_bs; d.out_cs = a->out_cs;
    d.add = a->add; d.add_bs = a->add_bs; d.add_cs = a->add_cs;
    d.part = a->part;
    d.gamma = blk->gamma[0];
    d.film = a->film + blk->film_aff[0];
    d.film_bs = a->film_bs;
    d.gate = a->gate;
    d.stats = a->stats; d.scale = a->scale;
    d.wH = static_cast<const float*>(blk->H[0].fwd);
    d.wres = static_cast<const float*>(blk->res_conv.fwd);
    d.wpo = static_cast<const float*>(blk->proj_out.fwd);
    d.ntH = pw_image_nt(blk->H[0], N); d.ntres = pw_image_nt(blk->res_conv, blk->res_conv.Cout);
    d.FT = a->F * a->T; d.S = a->S;
    d.n = (long)(N / PW_G) * d.FT;
    // algorithmic work, as the layer-by-layer path's (1,1) convs count it: z once (+ the init block's output), the H matrix and
    // the two-channel sides; 2 N^2 flop per position for H and 2 * 2 N for each projection
    const double px = (double)a->B * d.FT;
    const double bytes = 4.0 * (px * (N + (kind == 2 ? N + 2 : 2 + (a->add ? 2 : 0))) + (double)N * N + 4.0 * N);
    const double flops = 2.0 * px * ((double)N * N + 4.0 * N);
    BabeProfScope prof(BABE_SLOT_CONV11, bytes, flops, 2.0 * px * (double)N * N, stream);
    hipStream_t s = (hipStream_t)stream;
    switch (N / 32) {
        case 2: pw_launch<2>(kind == 1, d, a->B, s); break;
        case 3: pw_launch<3>(kind == 1, d, a->B, s); break;
        case 4: pw_launch<4>(kind == 1, d, a->B, s); break;
        case 5: pw_launch<5>(kind == 1, d, a->B, s); break;
        case 6: pw_launch<6>(kind == 1, d, a->B, s); break;
        case 7: pw_launch<7>(kind == 1, d, a->B, s); break;
        default: pw_launch<8>(kind == 1, d, a->B, s); break;
    }
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
