// Frequency encodings of the CQTDiff+ init blocks (AddFreqEncodingRFF, networks/cqtdiff+.py:213-263, concatenated at :754-761 in
// front of ResnetBlock(66 -> N, (1,1)) :675) WITHOUT the 64 extra channels: the encodings E[j][f] are constant over batch and time
// and only two bias-free (1,1) convs (proj_in, res_conv) read them, so their share of those convs is a table
//   Fb[co][f] = sum_j W[co][2 + j] * E[j][f]
// that the conv adds in its epilogue (babe_conv_args::fbias); the conv itself reads the 2 signal channels.  This file builds the
// table (after every weight change, in place) and, for training, the encoding columns of the weight gradient
//   dW[co][2 + j] = sum_f E[j][f] * sum_{b,t} g[b][co][f][t]
// per batch row.  Fixed-order sums, no atomics.  F = 64 bins per octave and 64 = 2 x 32 encodings, as in the reference.
#include "common.h"
#include "../../include/babe_hip.h"

namespace {

constexpr int FE_F = 64, FE_J = 64;

__global__ __launch_bounds__(64) void fenc_bias_kernel(const float* __restrict__ w, const float* __restrict__ emb, float* __restrict__ fb,
                                                       int ld_w) {
    const int co = blockIdx.x, f = threadIdx.x;
    const float* wr = w + (long)co * ld_w + 2;
    float s = 0.f;
    for (int j = 0; j < FE_J; ++j) s = __builtin_fmaf(wr[j], emb[j * FE_F + f], s);
    fb[co * FE_F + f] = s;
}

// one workgroup per (co, b): 4 threads per frequency row sum interleaved time steps, combined in order; then thread j < 64 contracts
// the 64 row sums with its encoding
__global__ __launch_bounds__(256) void fenc_wgrad_kernel(const float* __restrict__ g, long g_bs, long g_cs, const float* __restrict__ emb,
                                                         float alpha, float* __restrict__ rows, long rows_bs, int ld_row, int T) {
    __shared__ double part[FE_F][4];
    __shared__ double rs[FE_F];
    const int co = blockIdx.x, b = blockIdx.y;
    const int f = threadIdx.x >> 2, p = threadIdx.x & 3;
    const float* gr = g + (long)b * g_bs + (long)co * g_cs + (long)f * T;
    double s = 0.0;
    for (int t = p; t < T; t += 4) s += (double)gr[t];
    part[f][p] = s;
    __syncthreads();
    if (threadIdx.x < FE_F) rs[threadIdx.x] = ((part[threadIdx.x][0] + part[threadIdx.x][1]) + part[threadIdx.x][2]) + part[threadIdx.x][3];
    __syncthreads();
    if (threadIdx.x < FE_J) {
        const int j = threadIdx.x;
        double d = 0.0;
        for (int ff = 0; ff < FE_F; ++ff) d += (double)emb[j * FE_F + ff] * rs[ff];
        rows[(long)b * rows_bs + (long)co * ld_row + 2 + j] = alpha * (float)d;
    }
}

}  // namespace

extern "C" int babe_fenc_bias(const float* w, const float* emb, float* fb, int Cout, int ld_w, void* stream) {
    BABE_CHECK_ARG(w && emb && fb, "fenc_bias: null pointer");
    BABE_CHECK_ARG(Cout > 0 && ld_w >= 2 + FE_J, "fenc_bias: bad shape (Cout %d, ld_w %d: the weight rows hold 2 + 64 columns)", Cout, ld_w);
    hipLaunchKernelGGL(fenc_bias_kernel, dim3(Cout), dim3(64), 0, (hipStream_t)stream, w, emb, fb, ld_w);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_fenc_wgrad_rows(const float* g, long g_bs, long g_cs, const float* emb, float alpha, float* rows, long rows_bs,
                                    int ld_row, int B, int Cout, int F, int T, void* stream) {
    BABE_CHECK_ARG(g && emb && rows, "fenc_wgrad_rows: null pointer");
    BABE_CHECK_ARG(F == FE_F, "fenc_wgrad_rows: F = %d (the encodings cover 64 bins per octave)", F);
    BABE_CHECK_ARG(B > 0 && B <= 65535 && Cout > 0 && T > 0 && ld_row >= 2 + FE_J, "fenc_wgrad_rows: bad shape (B %d, Cout %d, T %d, ld_row %d)", B,
                   Cout, T, ld_row);
    BABE_CHECK_ARG(g_cs >= (long)FE_F * T && rows_bs >= (long)Cout * ld_row, "fenc_wgrad_rows: strides smaller than the tensors");
    hipLaunchKernelGGL(fenc_wgrad_kernel, dim3(Cout, B), dim3(256), 0, (hipStream_t)stream, g, g_bs, g_cs, emb, alpha, rows, rows_bs, ld_row, T);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
