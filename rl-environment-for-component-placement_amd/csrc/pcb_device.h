// pcb_device.h -- device-only helpers of the kernels: coherent loads, diagnostic stamps, bit rows, 16-byte plane emission, cross-lane scans
// Included by every unit of libpcbenv.so that defines a kernel (through pcb_team.h, pcb_geninst.h or pcb_policy_common.h); CDNA4 / gfx950 only.
// The parameter block and the state-block records are plain data: pcb_records.h, which the host units include without this file.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "pcb_records.h"

// Loads of data another stream's kernel (or a DMA) has written since this XCD last read the same addresses: instance
// records and the generator's counters.  Agent-scope loads (`sc1`) are served coherently; a plain load may hit a
// stale clean line in this XCD's L2.
__device__ inline u64 load_agent(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline unsigned load_agent(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int load_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store_agent(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// In-kernel stamps (cdna_hip_programming.md §7): only in a separate diagnostic build, written to a buffer nothing
// else reads; `PCBENV_STAMPS=1` in the environment allocates it, tools/kernel_stamps.py prints the phase profile.
#ifdef PCBENV_STAMPS
#define STAMP(k) do { if ((threadIdx.x & (NT - 1)) == 0 && p.dbg) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); p.dbg[(size_t)blockIdx.x * 32 + (k)] = t_; } } while (0)
#define STAMP_RT(k) do { if ((threadIdx.x & (NT - 1)) == 0 && p.dbg) { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); p.dbg[(size_t)blockIdx.x * 32 + (k)] = t_; } } while (0)
// accumulate elapsed shader cycles of a region / an arbitrary value into slot k (the kernel's first STAMP must zero it)
#define STAMP_T0() unsigned long long st0_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st0_) :: "memory")
#define STAMP_ACC_SINCE(k, dep) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory"); if ((threadIdx.x & (NT - 1)) == 0 && p.dbg) p.dbg[(size_t)blockIdx.x * 32 + (k)] += t_ - st0_; } while (0)
#define STAMP_ADD(k, v) do { if ((threadIdx.x & (NT - 1)) == 0 && p.dbg) p.dbg[(size_t)blockIdx.x * 32 + (k)] += (unsigned long long)(v); } while (0)
#define STAMP_ZERO(k) do { if ((threadIdx.x & (NT - 1)) == 0 && p.dbg) p.dbg[(size_t)blockIdx.x * 32 + (k)] = 0ull; } while (0)
// the stamps above index their rows by blockIdx.x: shift the table so that this team's rows are environment e's
#define STAMP_ROWS_BY_ENV(launch, e) DevParams p = (launch); if (p.dbg) p.dbg += ((long long)(e) - (long long)blockIdx.x) * 32
#else
#define STAMP(k) do { } while (0)
#define STAMP_RT(k) do { } while (0)
#define STAMP_T0() do { } while (0)
#define STAMP_ACC_SINCE(k, dep) do { } while (0)
#define STAMP_ADD(k, v) do { } while (0)
#define STAMP_ZERO(k) do { } while (0)
#define STAMP_ROWS_BY_ENV(launch, e) const DevParams &p = (launch)
#endif

// ---- cold fields of the parameter block ----
// PCB_COLD(p, field): a field of DevParams that only a terminal transition, the reset behind it or the terminal-list
// bookkeeping reads (reward weights and norms, the instance queue, the generator's counters, the list's arrays).  Held
// as a value from kernel entry, such a field occupies scalar registers through the whole plain transition, where the
// compiler parks it in a vector lane on the way in (profiles/step_head.txt).  The geometry-fixed builds of k_step --
// part 4 of pcb_layout::step_build_part, the only kernels of their units, with the block as first kernel argument at
// offset 0 -- load it from the kernel-argument segment where it is used instead: the pointer goes through an empty
// volatile asm, so the load can be neither merged with the entry loads nor hoisted out of the branch it stands in.
// Every other unit reads the field of the block as before (same device code).
#if defined(PCB_PART) && PCB_PART == 4
#define PCB_GEO64_UNIT 1  // this unit compiles the geometry-fixed builds of k_step and nothing else
template <class T> __device__ __forceinline__ T kernarg_field_at_use(unsigned offset) {
    typedef const __attribute__((address_space(4))) unsigned char *kernarg_ptr;
    kernarg_ptr k = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return *(const __attribute__((address_space(4))) T *)(k + offset);
}
// The kernel-argument segment of a launch is fresh memory: the first scalar load of each of its 64-byte lines misses
// the scalar cache, and the compiler reloads fields where they are used, one line and one wait at a time, along the
// head of a transition.  kernarg_warm() touches every line of the segment at kernel entry, all loads in flight
// together behind one wait, so that the loads further down hit.  BYTES: the size of the segment.
template <int BYTES> __device__ __forceinline__ void kernarg_warm() {
    static_assert(BYTES > 0x200 + 4 && BYTES <= 0x240, "one load per 64-byte line of the segment, and its last word");
    typedef const __attribute__((address_space(4))) unsigned char *kernarg_ptr;
    kernarg_ptr k = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned t0, t1, t2, t3, t4, t5, t6, t7, t8, t9;
    asm volatile("s_load_dword %0, %10, 0x0\n\ts_load_dword %1, %10, 0x40\n\ts_load_dword %2, %10, 0x80\n\ts_load_dword %3, %10, 0xc0\n\t"
                 "s_load_dword %4, %10, 0x100\n\ts_load_dword %5, %10, 0x140\n\ts_load_dword %6, %10, 0x180\n\ts_load_dword %7, %10, 0x1c0\n\t"
                 "s_load_dword %8, %10, 0x200\n\ts_load_dword %9, %10, %11\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3), "=&s"(t4), "=&s"(t5), "=&s"(t6), "=&s"(t7), "=&s"(t8), "=&s"(t9)
                 : "s"(k), "n"((BYTES - 4) & ~3));
}
#define PCB_COLD(p, field) kernarg_field_at_use<std::remove_cv_t<std::remove_reference_t<decltype((p).field)>>>((unsigned)offsetof(DevParams, field))
#else
#define PCB_GEO64_UNIT 0
#define PCB_COLD(p, field) ((p).field)
#endif


// ---- bit rows ----
template <int WW> struct Row;
template <> struct Row<1> {
    u64 a;
    __device__ static Row load(const u64 *p) { return Row{p[0]}; }
    __device__ void store(u64 *p) const { p[0] = a; }
    __device__ Row operator|(Row o) const { return Row{a | o.a}; }
    __device__ Row shr(int k) const { return Row{k >= 64 ? 0ull : a >> k}; }
    __device__ static Row zero() { return Row{0ull}; }
    __device__ bool any() const { return a != 0; }
    // valid = ~occ restricted to columns [0, n)
    __device__ Row free_below(int n) const { return Row{n <= 0 ? 0ull : (~a & (n >= 64 ? ~0ull : ((1ull << n) - 1ull)))}; }
};
template <> struct Row<2> {
    u64 a, b;
    __device__ static Row load(const u64 *p) { return Row{p[0], p[1]}; }
    __device__ void store(u64 *p) const { p[0] = a; p[1] = b; }
    __device__ Row operator|(Row o) const { return Row{a | o.a, b | o.b}; }
    __device__ Row shr(int k) const {
        if (k == 0) return *this;
        if (k >= 128) return Row{0ull, 0ull};
        if (k >= 64) return Row{b >> (k - 64), 0ull};
        return Row{(a >> k) | (b << (64 - k)), b >> k};
    }
    __device__ static Row zero() { return Row{0ull, 0ull}; }
    __device__ bool any() const { return (a | b) != 0; }
    __device__ Row free_below(int n) const {
        u64 ma = n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1ull));
        u64 mb = n <= 64 ? 0ull : (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull));
        return Row{~a & ma, ~b & mb};
    }
};

// OR_{k < pw} (row >> k): bit j set iff some cell j..j+pw-1 of the row is occupied (log-step doubling).
template <int WW> __device__ inline Row<WW> hfold(Row<WW> r, int pw) {
    Row<WW> f = r;
    int s = 1;
    while (2 * s <= pw) { f = f | f.shr(s); s *= 2; }
    if (s < pw) f = f | f.shr(pw - s);
    return f;
}

// 16-byte observation store, agent-scope write-through (`sc1`): every line written here is next read by another
// launch (usually on another XCD) or by the policy, never by this workgroup, so leaving it dirty in the XCD's L2
// only defers the write to the end-of-kernel release, where the whole grid waits for it (+5 % at c3).
// STREAM adds `nt`: when one launch writes well beyond the 256 MiB Infinity Cache, lines allocated there are
// evicted before anything reads them and only cost fabric traffic (c5, 3.1 GB per launch: +10..20 %; c3 at 65 536
// environments: 192 M -> 271 M env-steps/s), while below that size the cache absorbs the burst and streaming is the
// slower choice (c3 / c4 at 4 096 environments: -6 %).  pcbenv_create picks by bytes per launch (DevParams).
// The stores are raw buffer stores (buffer_store_dwordx4 ... sc1 [nt]) through a per-environment resource
// descriptor: the cache policy travels in the builtin's aux operand, so the compiler schedules them (and their
// gfx950 store-data wait states) itself, and the descriptor's byte count makes an out-of-range chunk a dropped
// store instead of a fault.  -DPCBENV_STORE_PLAIN keeps plain global stores for A/B runs.
typedef unsigned v4u __attribute__((ext_vector_type(4)));
#if defined(PCBENV_STORE_PLAIN)
struct ObsDst { unsigned char *base; };
__device__ inline ObsDst obs_dst(unsigned char *base, long long) { return ObsDst{base}; }
template <bool STREAM> __device__ inline void STORE16(const ObsDst &d, unsigned off, uint4 v) { *(uint4 *)(d.base + off) = v; }
#else
struct ObsDst { __amdgpu_buffer_rsrc_t rsrc; };
// base must be wave-uniform (it is: tensor pointer + blockIdx.x * per-environment bytes)
__device__ inline ObsDst obs_dst(unsigned char *base, long long bytes) {
    // The descriptor has to sit in scalar registers.  Where the compiler cannot prove base / bytes uniform it wraps every
    // store in a "waterfall" loop (readfirstlane x 4, compare, saveexec, branch -- per store); they ARE uniform, say so.
    const uintptr_t b = (uintptr_t)base;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    unsigned char *ub = (unsigned char *)(((uintptr_t)hi << 32) | lo);
    return ObsDst{__builtin_amdgcn_make_buffer_rsrc(ub, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000)};
}
#define PCBENV_AUX_SC1 16
#define PCBENV_AUX_NT 2
template <bool STREAM> __device__ inline void STORE16(const ObsDst &d, unsigned off, uint4 v) {
    const v4u w{v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(w, d.rsrc, (int)off, 0, STREAM ? (PCBENV_AUX_SC1 | PCBENV_AUX_NT) : PCBENV_AUX_SC1);
}
#endif

// 4 mask bits -> 4 bytes of 0/1
__device__ inline unsigned expand4(unsigned b) { return (b * 0x00204081u) & 0x01010101u; }
__device__ inline uint4 expand16(unsigned bits) {
    return make_uint4(expand4(bits & 15u), expand4((bits >> 4) & 15u), expand4((bits >> 8) & 15u), expand4((bits >> 12) & 15u));
}

__device__ inline void STORE16_dyn(const ObsDst &d, unsigned off, uint4 v, bool stream) { if (stream) STORE16<true>(d, off, v); else STORE16<false>(d, off, v); }
// value of `a` held by lane + s (0 beyond the wavefront): one cross-lane read per 32-bit half
__device__ inline u64 lane_down(u64 a, int s, int lane) {
    const int src = (lane + s) << 2;
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)(unsigned)(a >> 32));
    return lane + s < WAVE ? (((u64)hi << 32) | lo) : 0ull;
}
// Inclusive prefix sum over each group of G = 16, 32 or 64 consecutive lanes with DPP row shifts / row broadcasts (no LDS
// round trips): the wavefront's (sample_action) or, narrower, one per environment of the instance generator.
template <int G> __device__ inline int group_inclusive_scan(int x, int lane) {
    const int row = lane & 15;
    int t;
    t = __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false); if (row >= 1) x += t;   // row_shr:1
    t = __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false); if (row >= 2) x += t;   // row_shr:2
    t = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false); if (row >= 4) x += t;   // row_shr:4
    t = __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false); if (row >= 8) x += t;   // row_shr:8
    if (G >= 32) { t = __builtin_amdgcn_update_dpp(0, x, 0x142, 0xF, 0xF, false); if ((lane & 31) >= 16) x += t; }  // row_bcast:15
    if (G == 64) { t = __builtin_amdgcn_update_dpp(0, x, 0x143, 0xF, 0xF, false); if (lane >= 32) x += t; }         // row_bcast:31
    return x;
}

// Workgroups go to the eight XCDs round-robin (blockIdx.x % 8).  Environment of workgroup `block` (the environments'
// workgroups follow `head` others): XCD * B/8 + turn, so that each XCD -- each L2 -- owns a contiguous eighth of every
// tensor.  Rows smaller than a cache line (reward, done, info, actions, the compact features) and the ends of the
// others then share their lines with neighbours under the SAME L2, which merges them into whole-line writes; with
// environment = blockIdx.x every such line went to memory in up to eight pieces (c3: 19.65 -> 19.1 us per launch, c4
// 44.8 -> 44.3, same-box A/B in profiles/r3/ab_xcd_contiguous_environments.txt).  Any bijection serves: the
// environments are independent, and nothing else depends on which workgroup runs which.
__device__ inline int xcd_contiguous_env(int block, int head, int B) {
    if (B & 7) return block - head;
    const int x = block & 7, first = head + ((x - head) & 7);  // first: the XCD's first environment workgroup
    return x * (B >> 3) + (block - first) / 8;
}
