// The GroupNorm finalize and the fixed-order sum of a group's partial pairs, shared by the kernels that turn babe_gn_partial's
// sums into statistics (csrc/norm.hip, csrc/pw_block.hip), so that all of them round identically.
#pragma once
namespace {

// The one GroupNorm finalize: (sum, sum of squares) of a group of n elements -> mean, unbiased std (variance clamped at 0) and
// r = 1 / (std + eps).  gn_partial_kernel<true>, gn_finalize_kernel and scale_gelu_fin_kernel agree bit for bit through it.
struct GnStat {
    float mean, sd, r;
};
__device__ __forceinline__ GnStat gn_stat(double s0, double s1, long n, float eps) {
    const double mean = s0 / (double)n;
    double var = (s1 - (double)n * mean * mean) / (double)(n - 1);
    if (var < 0) var = 0;
    const float sd = (float)sqrt(var);
    return {(float)mean, sd, 1.f / (sd + eps)};
}
__device__ __forceinline__ void gn_stat_store(float* __restrict__ stats, int bg, const GnStat st) {
    stats[bg * 3 + 0] = st.mean;
    stats[bg * 3 + 1] = st.sd;
    stats[bg * 3 + 2] = st.r;
}

// the two sums of a 32-lane half-wave, to every lane of it
__device__ __forceinline__ void half_wave_sum2(double& s0, double& s1) {
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
        s0 += __shfl_xor(s0, o, 32);
        s1 += __shfl_xor(s1, o, 32);
    }
}
// The S partial pairs of a group, pairs row ... row + S - 1 of part, added by one half-wave: lane sub takes sub, sub + 32, ... in
// that order, then the shuffles.  P: const double*, or const volatile double* for pairs that other workgroups of the same
// launch wrote.
template <typename P>
__device__ __forceinline__ void gn_part_sum32(P part, long row, int S, int sub, double& s0, double& s1) {
    s0 = 0, s1 = 0;
    for (int q = sub; q < S; q += 32) {
        s0 += part[(row + q) * 2];
        s1 += part[(row + q) * 2 + 1];
    }
    half_wave_sum2(s0, s1);
}

}  // namespace
