// pcb_sample.hip -- the two plain (non-template) kernels of libpcbenv.so that serve every environment kind: k_sample
// (pcbenv_sample_actions: one uniformly drawn legal action per environment) and k_cursor_range (pcbenv_queue_cursors).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, like the per-kind units.
#include "pcb_sampler.h"
#include "pcb_launch.h"

__global__ __launch_bounds__(WAVE) void k_sample(DevParams p, int *__restrict__ actions, int fmt, u64 seed,
                                                 u64 first_env, u64 step_index) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const u64 *vm = (const u64 *)(p.state + (size_t)e * p.stateStride + p.offVm);
    int o, x, y;
    sample_action(vm, p, (int)first_env + e, lane, seed, step_index, &o, &x, &y);
    if (lane == 0) {
        if (fmt == PCBENV_ACTION_FLAT) actions[e] = o * p.H * p.W + x * p.W + y;
        else { actions[3 * e] = o; actions[3 * e + 1] = x; actions[3 * e + 2] = y; }
    }
}

// min / max of the per-environment queue cursors (one small workgroup; B <= a few thousand headers)
__global__ __launch_bounds__(256) void k_cursor_range(DevParams p, unsigned *out) {
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    for (int e = threadIdx.x; e < p.B; e += 256) {
        const unsigned c = load_agent(p.cursor_pub + e);  // not the state block: that copy is only coherent on its own XCD
        lo = min(lo, c); hi = max(hi, c);
    }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, (unsigned)__shfl_xor((int)lo, o)); hi = max(hi, (unsigned)__shfl_xor((int)hi, o)); }
    __shared__ unsigned slo[4], shi[4];
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) { lo = min(lo, slo[w]); hi = max(hi, shi[w]); }
        out[0] = lo; out[1] = hi;
    }
}

int pcb_launch_sample(const SampleLaunch &a) {
    hipLaunchKernelGGL(k_sample, dim3(a.d.B), dim3(WAVE), 0, a.stream, a.d, a.actions, a.fmt, a.seed, a.first_env, a.step_index);
    return 0;
}
int pcb_launch_cursor_range(const DevParams &d, unsigned *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_cursor_range, dim3(1), dim3(256), 0, stream, d, out);
    return 0;
}
