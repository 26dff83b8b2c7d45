// Development only (never part of the product build): where the shader cycles of the WORKGROUP walk's step go.
// Built with SYMACCEL_TUNE_AAC_QUAD=2 (a tuned side build, symphonia_amd/build/tuned/), read back by tools/aac_step_probe.py.
//
// aac.hip includes this file in front of aac_synth_quad_kernel; the kernel's text is not touched: the three things a step can
// stand still in are calls -- wg_sync_lds() twice per step and channel (barrier 1: the delay lines are in their slots; barrier 2:
// the slots are free), settle_prefetch() once (the wait for the prefetched lines) -- and the macros below wrap a cycle counter
// around each.  The accumulators live in 128 bytes of LDS (zeroed where the kernel calls __syncthreads(), in front of the walk);
// every 32 steps lane 0 of each wavefront writes its running totals over the first PCM frame of the segment, which CORRUPTS that
// frame by construction (eight dwords at word 16 * wave):
//     tag 0x57e9c10c | barrier pairs so far | cycles in barrier 1 | in barrier 2 | in the prefetch wait | cycles since the walk began
//     | HW_ID | XCC_ID
// A source whose loop waits for the prefetch implicitly (no settle_prefetch: the loop header's `s_waitcnt vmcnt(0)` of the walk
// before the uniform step) is measured with SYM_PROBE_TOP(line, sb_next) placed at the top of its loop: the same claim, timed.
#pragma once

struct QuadProbeAcc {
    unsigned long long pairs, b1, b2, wait, t0, calls, pad0, pad1;
};

__device__ __forceinline__ QuadProbeAcc *quad_probe_acc(int wave) {
    __shared__ QuadProbeAcc acc[4];
    return &acc[wave & 3];
}

__device__ __forceinline__ void quad_probe_begin(int wave, int lane) {
    QuadProbeAcc *a = quad_probe_acc(wave);
    if (lane == 0) {
        a->pairs = a->b1 = a->b2 = a->wait = a->calls = 0ull;
        a->t0 = __builtin_readcyclecounter();
    }
    (__syncthreads)();
}

__device__ __forceinline__ void quad_probe_sync(int wave, int lane, float *first_frame) {
    QuadProbeAcc *a = quad_probe_acc(wave);
    const unsigned long long c0 = __builtin_readcyclecounter();
    (wg_sync_lds)();
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (lane == 0) {
        const unsigned long long k = a->calls;
        a->calls = k + 1;
        if ((k & 1ull) == 0ull) {
            a->b1 += c1 - c0;
        } else {
            a->b2 += c1 - c0;
            const unsigned long long pairs = a->pairs + 1;
            a->pairs = pairs;
            if ((pairs & 31ull) == 0ull) {
                unsigned hw, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                uint4 *o = reinterpret_cast<uint4 *>(first_frame) + 4 * (wave & 3);
                o[0] = make_uint4(0x57e9c10cu, (unsigned)pairs, (unsigned)a->b1, (unsigned)a->b2);
                o[1] = make_uint4((unsigned)a->wait, (unsigned)(c1 - a->t0), hw, xcc);
            }
        }
    }
}

template <typename Claim>
__device__ __forceinline__ void quad_probe_wait(int wave, int lane, Claim claim) {
    const unsigned long long c0 = __builtin_readcyclecounter();
    claim();
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (lane == 0) quad_probe_acc(wave)->wait += c1 - c0;
}

// (the names on the right are the kernel's own: the macros expand inside it)
#define __syncthreads() quad_probe_begin(wave, lane)
#define wg_sync_lds() quad_probe_sync(wave, lane, pcm + (chain_base0 + (size_t)t_begin) * 1024)
#define settle_prefetch(l) quad_probe_wait(wave, lane, [&]() { (settle_prefetch)(l); })
#define SYM_PROBE_TOP(l, sb)                                                                                                     \
    quad_probe_wait(wave, lane, [&]() {                                                                                          \
        asm volatile("" : : "v"(l[0].x), "v"(l[0].y), "v"(l[1].x), "v"(l[1].y), "v"(l[2].x), "v"(l[2].y), "v"(l[3].x), "v"(l[3].y), \
                     "v"(l[4].x), "v"(l[4].y), "v"(l[5].x), "v"(l[5].y), "v"(l[6].x), "v"(l[6].y), "v"(l[7].x), "v"(l[7].y), "v"(sb)); \
    })
