// The one workgroup reduction of the 3-D units (pl_3d.hip, pl_step3.hip, pl_mic3.hip): K slots per thread, each with an operation that
// is a compile-time constant (the type OPS: R3Ops or R3All below), 256 threads = four waves of 64 lanes.  A slot goes through a
// shuffle tree over the lanes (offsets 32, 16, ..., 1), then the four wave results are combined as ((w0 o w1) o w2) o w3, and slot q
// of workgroup b lands in part[K b + q].  The order is part of the contract: the floating-point sums of the Krylov reductions depend on it.
//
// k_r3_finish combines such partials on the device.  It is for slots whose result does not depend on the order: minima and maxima
// (fmin / fmax drop a NaN in any order) and counts held in a double (exact in any order below 2^53).  A floating-point SUM whose bits
// matter must not go through it as it stands: the host adds those partials, block 0 upward (sum_partials3 in pl_3d.hip).
//
// (r3_block takes the thread's flat index rather than lane and wave apart, and r3_wave its value by reference: written the other way
// the all-sum kernels of pl_3d.hip no longer compile to the code they had with this loop written out in place.)
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

enum { R3_SUM = 0, R3_MIN = 1, R3_MAX = 2 };
__device__ inline double r3_comb(int op, double a, double b) { return op == R3_SUM ? a + b : (op == R3_MIN ? fmin(a, b) : fmax(a, b)); }
__device__ inline double r3_unit(int op) { return op == R3_SUM ? 0.0 : (op == R3_MIN ? INFINITY : -INFINITY); }
// the 64 lanes of a wave -> lane 0
__device__ inline void r3_wave(int op, double& x) {
    for (int o = 32; o > 0; o >>= 1) x = r3_comb(op, x, __shfl_down(x, o, 64));
}
// The operations of K slots, as a type: R3Ops<R3_MIN, R3_MAX, ...> slot by slot, R3All<R3_SUM, 5> the same one for all
template <int... O> struct R3Ops {
    static constexpr int K = sizeof...(O);
    static constexpr int op(int q) { constexpr int t[K] = {O...}; return t[q]; }
};
template <int OP, int N> struct R3All {
    static constexpr int K = N;
    static constexpr int op(int) { return OP; }
};
// acc[q] of thread t (0 .. 255: lane t % 64 of wave t / 64, however the grid numbers its threads) of workgroup `block` -> part[K block + q]
template <class OPS>
__device__ inline void r3_block(const double (&acc)[OPS::K], unsigned t, unsigned block, double* __restrict__ part) {
    constexpr int K = OPS::K;
    __shared__ double sh[K][4];
    const unsigned lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int q = 0; q < K; q++) {
        double x = acc[q];
        r3_wave(OPS::op(q), x);
        if (lane == 0) sh[q][wave] = x;
    }
    __syncthreads();
    if (t < K) {
        const int op = OPS::op(t);
        part[K * block + t] = r3_comb(op, r3_comb(op, r3_comb(op, sh[t][0], sh[t][1]), sh[t][2]), sh[t][3]);
    }
}
// Workgroup g combines the partials [g chunk, (g + 1) chunk) of nb: thread t those at t, t + 256, ... of its chunk, then the 256 threads as
// above -> out[K g + q].  One workgroup with chunk = nb finishes a short list; a long one takes two launches, G workgroups and then one
// over their G results.
template <class OPS>
__global__ __launch_bounds__(256) void k_r3_finish(long long nb, long long chunk, const double* __restrict__ part, double* __restrict__ out) {
    constexpr int K = OPS::K;
    const long long b0 = blockIdx.x * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
    double acc[K];
#pragma unroll
    for (int q = 0; q < K; q++) acc[q] = r3_unit(OPS::op(q));
    for (long long b = b0 + threadIdx.x; b < b1; b += 256) {
#pragma unroll
        for (int q = 0; q < K; q++) acc[q] = r3_comb(OPS::op(q), acc[q], part[(size_t)K * b + q]);
    }
    r3_block<OPS>(acc, threadIdx.x, blockIdx.x, out);
}
