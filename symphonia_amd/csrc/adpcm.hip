// ADPCM (MS, IMA WAV, IMA QT): packet bytes to PCM, the whole numeric decode of symphonia-codec-adpcm on the device.
//
//   codec_ms.rs:89-99        expand_nibble: (s1 * c1 + s2 * c2) / 256 + signed_nibble * delta, clamp_i16, delta = max(16, T[n] * delta / 256)
//   codec_ms.rs:101-136      decode_mono / decode_stereo: the preamble (7 / 14 bytes), sample2 then sample1, upper nibble first
//   common_ima.rs:38-48      expand_nibble: ((2 * (n & 7) + 1) * STEP[idx]) >> 3, clamp_i16, idx = clamp(idx + INDEX[n], 0, 88)
//   codec_ima_wav.rs:14-65   4-byte preamble per channel, lower nibble first, stereo in 4-byte groups per channel
//   codec_ima_qt.rs:14-47    big-endian preamble, 32 data bytes, stereo = two mono blocks one after the other
//
// Every block carries its own predictor state (lib.rs:217-219: reset() is empty), so a block is the unit of work and a LANE owns a block:
// the recurrence is serial inside a block, and a launch holds thousands of blocks.  A stereo block runs its two channels in one lane,
// two independent dependency chains.  A tile is 64 blocks, one wavefront:
//
//   refill   the wavefront loads the next 64 bytes of each of its 64 blocks into an LDS image, lanes side by side along a block's bytes
//            (16-byte loads of the aligned 16-byte units that cover the piece; a unit that reaches outside the input is loaded bytewise);
//            the image's row pitch is an odd number of dwords, so the lanes walking their own rows fall on different banks;
//   step     every lane takes 8 bytes (16 nibbles) of its row, a dword at a time, and writes the 16 samples into its row of an LDS ring
//            that stands for the output bytes around the position it has reached (byte b of a run sits at (b + the run's global address)
//            mod the ring size, so a 16-byte unit of the ring is a 16-byte aligned unit of global memory);
//   flush    the wavefront writes out the ring's completed 16-byte units, lanes side by side along a run; the up to 15 bytes at either
//            end of a run that do not fill an aligned unit leave in narrower stores, once per run.
//
// Global memory is never touched at a lane stride of one block, except for those run ends and the status bytes.
//
// Overflow rule (MS): delta can triple per nibble, so arbitrary bytes overflow i32 within tens of samples; the reference's release build
// wraps.  signed_nibble * delta, the sum with the prediction and T[n] * delta are computed in uint32_t (two's complement wrapping, no
// signed-overflow UB); the two divisions by 256 are truncating signed divisions of the wrapped values.  s1 * c1 + s2 * c2 cannot
// overflow (|s| <= 2^15, |c| <= 2^9), IMA cannot overflow at all.
//
// A block whose preamble the reference rejects (MS predictor index > 6: Unsupported, status 1; IMA WAV step index > 88: DecodeError,
// status 2) decodes to silence -- the value the native zero converts to in the output format.
//
// This file is part of the translation unit of batch_copy.hip (its last line includes it): the list of .hip sources is pinned by
// tests/test_build.py and by the emulation build.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "symaccel_internal.h"

namespace symaccel {

namespace {

constexpr unsigned kAdpcmLanes = 64;     // blocks of a tile
constexpr unsigned kAdpcmInPitch = 25;   // dwords: 6 units of 16 bytes (80 bytes at any alignment) + 1: odd
constexpr unsigned kAdpcmRing = 128;     // bytes of output ring per lane (split in two for the two planes of a native stereo block)
constexpr unsigned kAdpcmOutPitch = 33;  // dwords: the ring + 1: odd
constexpr unsigned kAdpcmTabStep = 0, kAdpcmTabAdapt = 96, kAdpcmTabC1 = 112, kAdpcmTabC2 = 120;

// common_ima.rs:19-30 IMA_STEP_TABLE | codec_ms.rs:15-18 MS_ADAPTATION_TABLE | codec_ms.rs:20-21 MS_ADAPT_COEFFS1 / 2 (copied into LDS by
// every workgroup: the lookups are per lane and sit inside the recurrence)
__device__ const int32_t kAdpcmTables[128] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209,
    230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749,
    3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623,
    27086, 29794, 32767, 0, 0, 0, 0, 0, 0, 0,
    230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230,
    256, 512, 0, 192, 240, 460, 392, 0,
    0, -256, 0, 64, 0, -208, -232, 0};

struct AdpcmArgs {
    const uint8_t *bytes;
    uint8_t *pcm;
    uint8_t *status;  // may be null
    size_t block_pitch, n_blocks, n_tiles;
    unsigned fpb, block_bytes;
    uint32_t flip, shr, f32;  // a sample s (i16) leaves as ((s << 16) ^ flip) >> shr, or as the f32 s / 32768
};

struct AdpcmChain {
    int32_t a, b, c1, c2, d;  // MS: sample1, sample2, coeff1, coeff2, delta; IMA: predictor, step index
};

__device__ __forceinline__ int32_t adpcm_clamp16(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// x / 256 of Rust (truncation toward zero)
__device__ __forceinline__ int32_t adpcm_div256(int32_t x) { return (int32_t)((uint32_t)x + (uint32_t)((x >> 31) & 255)) >> 8; }

// codec_ms.rs:89-99
__device__ __forceinline__ int32_t adpcm_ms_nibble(AdpcmChain &s, uint32_t n, const int32_t *tab) {
    const uint32_t sn = (n & 8u) ? n - 16u : n;
    const int32_t lin = adpcm_div256(s.a * s.c1 + s.b * s.c2);
    const int32_t p = (int32_t)((uint32_t)lin + sn * (uint32_t)s.d);
    s.b = s.a;
    s.a = adpcm_clamp16(p);
    const int32_t d = adpcm_div256((int32_t)((uint32_t)tab[kAdpcmTabAdapt + n] * (uint32_t)s.d));
    s.d = d < 16 ? 16 : d;
    return s.a;
}

// common_ima.rs:38-48 (IMA_INDEX_TABLE: -1 for n & 7 < 4, else 2, 4, 6, 8 -- looked up in a packed word)
__device__ __forceinline__ int32_t adpcm_ima_nibble(AdpcmChain &s, uint32_t n, const int32_t *tab) {
    const int32_t step = tab[kAdpcmTabStep + s.b];
    const int32_t diff = (int32_t)((2u * (n & 7u) + 1u) * (uint32_t)step) >> 3;
    s.a = adpcm_clamp16((n & 8u) ? s.a - diff : s.a + diff);
    const int32_t adj = (n & 4u) ? (int32_t)((0x08060402u >> (8u * (n & 3u))) & 0xffu) : -1;
    const int32_t i = s.b + adj;
    s.b = i < 0 ? 0 : (i > 88 ? 88 : i);
    return s.a;
}

__device__ __forceinline__ uint32_t adpcm_ld_byte(const uint32_t *img, unsigned off) { return (img[off >> 2] >> (8u * (off & 3u))) & 0xffu; }
__device__ __forceinline__ uint32_t adpcm_ld_dword(const uint32_t *img, unsigned off) {
    const uint64_t two = ((uint64_t)img[(off >> 2) + 1] << 32) | img[off >> 2];
    return (uint32_t)(two >> (8u * (off & 3u)));
}
__device__ __forceinline__ int32_t adpcm_i16(uint32_t lo, uint32_t hi) { return (int32_t)(int16_t)(uint16_t)(lo | (hi << 8)); }

// Bytes [at, at + n) of each of the tile's `nlive` blocks (n <= N <= 80) into the input image: row r holds the aligned 16-byte units that
// cover them, so the byte at `at + x` of block r is byte ((address of the block + at) & 15) + x of its row.
template <unsigned N>
__device__ __forceinline__ void adpcm_refill(const AdpcmArgs &a, size_t b0, unsigned nlive, unsigned at, unsigned n, uint32_t *in_img) {
    constexpr unsigned UPR = (N + 30u) / 16u;  // units a row can need
    const uintptr_t lo = reinterpret_cast<uintptr_t>(a.bytes), hi = lo + (a.n_blocks - 1) * a.block_pitch + a.block_bytes;
#pragma unroll
    for (unsigned it = 0; it < UPR; ++it) {
        const unsigned idx = threadIdx.x + kAdpcmLanes * it, r = idx / UPR, k = idx - r * UPR;
        if (r >= nlive) continue;
        const uintptr_t start = lo + (b0 + r) * a.block_pitch + at, unit = (start & ~(uintptr_t)15) + 16u * k;
        if (unit >= start + n) continue;
        uint4 v;
        if (unit >= lo && unit + 16u <= hi) {
            v = *reinterpret_cast<const uint4 *>(a.bytes + (unit - lo));  // (an offset from the kernel's own pointer: a global load, not a flat one)
        } else {  // the first or the last unit of the whole input
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (unsigned j = 0; j < 16u; ++j)
                if (unit + j >= lo && unit + j < hi) w[j >> 2] |= (uint32_t)a.bytes[unit + j - lo] << (8u * (j & 3u));
            v = uint4{w[0], w[1], w[2], w[3]};
        }
        uint32_t *row = in_img + r * kAdpcmInPitch + 4u * k;
        row[0] = v.x;
        row[1] = v.y;
        row[2] = v.z;
        row[3] = v.w;
    }
}

// CODEC: SYMACCEL_ADPCM_*; CH: 1 or 2; SB: bytes of an output sample, 0 = the native planes pcm[block][channel][fpb] of i32
template <int CODEC, unsigned CH, unsigned SB>
__global__ __launch_bounds__(kAdpcmLanes) void adpcm_decode_kernel(const AdpcmArgs a) {
    constexpr bool MS = CODEC == SYMACCEL_ADPCM_MS, QT = CODEC == SYMACCEL_ADPCM_IMA_QT;
    constexpr unsigned HB = MS ? 7u * CH : (QT ? 2u : 4u * CH);  // bytes in front of the first data byte
    constexpr unsigned H = MS ? 2u : (QT ? 0u : 1u);             // frames the preamble itself holds
    constexpr unsigned F = 16u / CH;                             // frames of a step
    constexpr unsigned NR = SB == 0 ? CH : 1u;                   // output runs of a block: its planes, or its interleaved frames
    constexpr unsigned BPF = SB == 0 ? 4u : CH * SB;             // bytes of a frame in a run
    constexpr unsigned RING = kAdpcmRing / NR;
    constexpr unsigned UPS = (F * BPF + 2u * BPF + 15u) / 16u;   // 16-byte units a run can complete in one step
    static_assert(F * BPF + 2u * BPF + 15u <= RING, "a step's bytes and what is left in front of them fit the ring");
    __shared__ int32_t tab[128];
    __shared__ uint32_t in_img[kAdpcmLanes * kAdpcmInPitch];
    __shared__ uint32_t out_img[kAdpcmLanes * kAdpcmOutPitch];
    const unsigned tid = threadIdx.x;
    tab[tid] = kAdpcmTables[tid];
    tab[tid + 64u] = kAdpcmTables[tid + 64u];
    const unsigned fpb = a.fpb, run_bytes = fpb * BPF;
    const unsigned nsteps = fpb > H + F ? (fpb - H + F - 1u) / F : 1u;
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(a.bytes), out0 = reinterpret_cast<uintptr_t>(a.pcm);
    const uint32_t *my_in = in_img + tid * kAdpcmInPitch;
    uint32_t *my_out = out_img + tid * kAdpcmOutPitch;
    uint8_t *my_out8 = reinterpret_cast<uint8_t *>(my_out);

    for (size_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const size_t b0 = tile * kAdpcmLanes;
        const unsigned nlive = a.n_blocks - b0 < kAdpcmLanes ? (unsigned)(a.n_blocks - b0) : kAdpcmLanes;
        const bool live = tid < nlive;
        const uintptr_t my_block = in0 + (b0 + (live ? tid : 0u)) * a.block_pitch;
        unsigned my_phase[NR];  // where the lane's runs start inside an aligned 16-byte unit
#pragma unroll
        for (unsigned c = 0; c < NR; ++c) my_phase[c] = (unsigned)((out0 + ((b0 + tid) * NR + c) * run_bytes) & 15u);

        // one sample into the lane's ring
        auto put = [&](unsigned c, unsigned f, int32_t s, bool bad) {
            if (bad) s = 0;
            const uint32_t w = a.f32 ? __float_as_uint((float)s * 0.000030517578125f) : (((uint32_t)s << 16) ^ a.flip) >> a.shr;
            if constexpr (SB == 0) {
                my_out[c * (RING / 4u) + (((my_phase[c] + f * 4u) & (RING - 1u)) >> 2)] = w;
            } else {
                const unsigned pos = my_phase[0] + (f * CH + c) * SB;
                if constexpr (SB == 4) my_out[(pos & (RING - 1u)) >> 2] = w;
                else if constexpr (SB == 2) *reinterpret_cast<uint16_t *>(my_out8 + (pos & (RING - 1u))) = (uint16_t)w;
                else if constexpr (SB == 1) my_out8[pos & (RING - 1u)] = (uint8_t)w;
                else {
                    my_out8[pos & (RING - 1u)] = (uint8_t)w;
                    my_out8[(pos + 1u) & (RING - 1u)] = (uint8_t)(w >> 8);
                    my_out8[(pos + 2u) & (RING - 1u)] = (uint8_t)(w >> 16);
                }
            }
        };

        // ---- the preamble(s)
        __syncthreads();  // (the tables; the previous tile's last flush)
        if constexpr (QT) adpcm_refill<80>(a, b0, nlive, 0u, 34u * CH, in_img);
        else adpcm_refill<16>(a, b0, nlive, 0u, HB, in_img);
        __syncthreads();
        AdpcmChain st[CH];
        unsigned code = 0;
        {
            const unsigned ph = (unsigned)(my_block & 15u);
#pragma unroll
            for (unsigned c = 0; c < CH; ++c) {
                if constexpr (MS) {  // codec_ms.rs:47-87: the fields of the two channels alternate
                    const uint32_t pi = adpcm_ld_byte(my_in, ph + c);
                    if (pi > 6u) code = 1;
                    st[c].c1 = tab[kAdpcmTabC1 + (pi > 6u ? 0u : pi)];
                    st[c].c2 = tab[kAdpcmTabC2 + (pi > 6u ? 0u : pi)];
                    const unsigned o = ph + CH + 2u * c;
                    st[c].d = adpcm_i16(adpcm_ld_byte(my_in, o), adpcm_ld_byte(my_in, o + 1u));
                    st[c].a = adpcm_i16(adpcm_ld_byte(my_in, o + 2u * CH), adpcm_ld_byte(my_in, o + 2u * CH + 1u));
                    st[c].b = adpcm_i16(adpcm_ld_byte(my_in, o + 4u * CH), adpcm_ld_byte(my_in, o + 4u * CH + 1u));
                } else if constexpr (QT) {  // codec_ima_qt.rs:14-22
                    const uint32_t h = (adpcm_ld_byte(my_in, ph + 34u * c) << 8) | adpcm_ld_byte(my_in, ph + 34u * c + 1u);
                    st[c].a = (int32_t)(int16_t)(uint16_t)(h & 0xff80u);
                    st[c].b = (int32_t)((h & 0x7fu) > 88u ? 88u : (h & 0x7fu));
                } else {  // codec_ima_wav.rs:14-25
                    const unsigned o = ph + 4u * c;
                    st[c].a = adpcm_i16(adpcm_ld_byte(my_in, o), adpcm_ld_byte(my_in, o + 1u));
                    const uint32_t i = adpcm_ld_byte(my_in, o + 2u);
                    if (i > 88u) code = 2;
                    st[c].b = (int32_t)(i > 88u ? 88u : i);
                }
            }
        }
        const bool bad = code != 0;
        if (live && a.status) a.status[b0 + tid] = (uint8_t)code;
#pragma unroll
        for (unsigned c = 0; c < CH; ++c) {
            if constexpr (MS) {  // codec_ms.rs:107-108, 124-127
                put(c, 0u, st[c].b, bad);
                put(c, 1u, st[c].a, bad);
            } else if constexpr (!QT) {
                put(c, 0u, st[c].a, bad);  // codec_ima_wav.rs:34, 49-50
            }
        }
        if constexpr (!QT) __syncthreads();  // (the first piece of data replaces the preamble in the image)

        // ---- the steps
        unsigned in_phase = (unsigned)(my_block & 15u);  // (QT: the whole block is in the image)
        for (unsigned s = 0; s < nsteps; ++s) {
            uint32_t w0, w1;
            if constexpr (QT) {
                w0 = adpcm_ld_dword(my_in, in_phase + 2u + (CH == 1 ? 8u : 4u) * s);
                w1 = adpcm_ld_dword(my_in, in_phase + (CH == 1 ? 6u + 8u * s : 36u + 4u * s));
            } else {
                const unsigned at = HB + 8u * s;
                if ((s & 7u) == 0) {  // (every lane is past its reads of the previous piece: the barrier behind the last flush)
                    const unsigned left = at < a.block_bytes ? a.block_bytes - at : 0u;
                    adpcm_refill<64>(a, b0, nlive, at, left < 64u ? left : 64u, in_img);
                    in_phase = (unsigned)((my_block + at) & 15u);
                    __syncthreads();
                }
                w0 = adpcm_ld_dword(my_in, in_phase + 8u * (s & 7u));
                w1 = adpcm_ld_dword(my_in, in_phase + 8u * (s & 7u) + 4u);
            }
            const unsigned f0 = H + s * F;
#pragma unroll
            for (unsigned i = 0; i < 8u; ++i) {
                const uint32_t byte = ((i < 4u ? w0 : w1) >> (8u * (i & 3u))) & 0xffu, lo_n = byte & 15u, hi_n = byte >> 4;
                if constexpr (MS && CH == 1) {  // codec_ms.rs:109-113
                    if (f0 + 2u * i < fpb) put(0u, f0 + 2u * i, adpcm_ms_nibble(st[0], hi_n, tab), bad);
                    if (f0 + 2u * i + 1u < fpb) put(0u, f0 + 2u * i + 1u, adpcm_ms_nibble(st[0], lo_n, tab), bad);
                } else if constexpr (MS) {  // codec_ms.rs:129-133
                    if (f0 + i < fpb) {
                        put(0u, f0 + i, adpcm_ms_nibble(st[0], hi_n, tab), bad);
                        put(CH - 1u, f0 + i, adpcm_ms_nibble(st[CH - 1u], lo_n, tab), bad);
                    }
                } else {  // codec_ima_wav.rs:35-39, 51-62; codec_ima_qt.rs:32-36: a dword is eight samples of one channel
                    const unsigned c = CH == 1 ? 0u : i / 4u, f = f0 + 2u * (CH == 1 ? i : (i & 3u));
                    if (f < fpb) put(c, f, adpcm_ima_nibble(st[c], lo_n, tab), bad);
                    if (f + 1u < fpb) put(c, f + 1u, adpcm_ima_nibble(st[c], hi_n, tab), bad);
                }
            }
            __syncthreads();

            // ---- flush: the aligned 16-byte units of every run that this step completed
            const unsigned done0 = s == 0 ? 0u : (f0 < fpb ? f0 : fpb) * BPF, done1 = (f0 + F < fpb ? f0 + F : fpb) * BPF;
#pragma unroll
            for (unsigned it = 0; it < NR * UPS; ++it) {
                const unsigned idx = tid + kAdpcmLanes * it, run = idx / UPS, k = idx - run * UPS;
                if (run >= nlive * NR) continue;
                const uintptr_t g = out0 + (b0 * NR + run) * (uintptr_t)run_bytes;
                const unsigned phase = (unsigned)(g & 15u), first = (phase + 15u) >> 4;
                const unsigned u0 = (phase + done0) >> 4, u = (u0 > first ? u0 : first) + k;
                if (u >= (phase + done1) >> 4) continue;
                const uint32_t *ring = out_img + (run / NR) * kAdpcmOutPitch + (run % NR) * (RING / 4u) + (((16u * u) & (RING - 1u)) >> 2);
                *reinterpret_cast<uint4 *>(a.pcm + (g - out0 - phase + 16u * (uintptr_t)u)) = uint4{ring[0], ring[1], ring[2], ring[3]};
            }
            // ---- the ends of a run that fill no aligned unit: its first bytes after the first step, its last after the last
            if (s == 0 || s + 1u == nsteps) {
                constexpr unsigned G = (SB == 0 || SB == 4) ? 4u : (SB == 2 ? 2u : 1u);  // bytes per edge store
#pragma unroll
                for (unsigned c = 0; c < NR; ++c) {
                    if (!live) continue;
                    const uintptr_t g = out0 + ((b0 + tid) * NR + c) * (uintptr_t)run_bytes;
                    const unsigned phase = my_phase[c], first = (phase + 15u) >> 4, last = (phase + run_bytes) >> 4;
                    const unsigned head = ((16u - phase) & 15u) < run_bytes ? ((16u - phase) & 15u) : run_bytes;
                    const unsigned tail = last >= first ? 16u * last - phase : run_bytes;
                    const uint8_t *ring8 = my_out8 + c * RING;
                    for (unsigned pass = 0; pass < 2u; ++pass) {
                        if (pass == 0 ? s != 0 : s + 1u != nsteps) continue;
                        const unsigned from = pass == 0 ? 0u : tail, to = pass == 0 ? head : run_bytes;
                        // (kept from the loop vectoriser: at most 15 bytes, and the ring position wraps)
#pragma clang loop vectorize(disable) interleave(disable)
                        for (unsigned y = from; y < to; y += G) {
                            const unsigned pos = (phase + y) & (RING - 1u);
                            uint8_t *to = a.pcm + (g - out0 + y);
                            if constexpr (G == 4) *reinterpret_cast<uint32_t *>(to) = *reinterpret_cast<const uint32_t *>(ring8 + pos);
                            else if constexpr (G == 2) *reinterpret_cast<uint16_t *>(to) = *reinterpret_cast<const uint16_t *>(ring8 + pos);
                            else *to = ring8[pos];
                        }
                    }
                }
            }
            __syncthreads();  // (the next step writes where these units were; the next refill replaces the piece just read)
        }
    }
}

template <int CODEC, unsigned CH>
void adpcm_launch_sb(unsigned sb, dim3 grid, hipStream_t stream, const AdpcmArgs &a) {
    switch (sb) {
    case 0: hipLaunchKernelGGL((adpcm_decode_kernel<CODEC, CH, 0>), grid, dim3(kAdpcmLanes), 0, stream, a); break;
    case 1: hipLaunchKernelGGL((adpcm_decode_kernel<CODEC, CH, 1>), grid, dim3(kAdpcmLanes), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((adpcm_decode_kernel<CODEC, CH, 2>), grid, dim3(kAdpcmLanes), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((adpcm_decode_kernel<CODEC, CH, 3>), grid, dim3(kAdpcmLanes), 0, stream, a); break;
    default: hipLaunchKernelGGL((adpcm_decode_kernel<CODEC, CH, 4>), grid, dim3(kAdpcmLanes), 0, stream, a); break;
    }
}

template <int CODEC>
void adpcm_launch_ch(unsigned channels, unsigned sb, dim3 grid, hipStream_t stream, const AdpcmArgs &a) {
    if (channels == 1) adpcm_launch_sb<CODEC, 1>(sb, grid, stream, a);
    else adpcm_launch_sb<CODEC, 2>(sb, grid, stream, a);
}

}  // namespace

// (the caller has checked the shape, the pointers' alignment and the sizes: symaccel_adpcm_decode_device)
int launch_adpcm_decode(symaccel_ctx *ctx, hipStream_t stream, const void *d_bytes, size_t block_pitch, size_t n_blocks, int codec, unsigned channels,
                        unsigned frames_per_block, void *d_pcm, int out_fmt, uint8_t *d_status) {
    if (n_blocks == 0) return SYMACCEL_OK;
    AdpcmArgs a;
    a.bytes = static_cast<const uint8_t *>(d_bytes);
    a.pcm = static_cast<uint8_t *>(d_pcm);
    a.status = d_status;
    a.block_pitch = block_pitch;
    a.n_blocks = n_blocks;
    a.n_tiles = (n_blocks + kAdpcmLanes - 1) / kAdpcmLanes;
    a.fpb = frames_per_block;
    a.block_bytes = (unsigned)adpcm_block_bytes(codec, channels, frames_per_block);
    const unsigned sb = out_fmt == 0 ? 0u : (unsigned)symaccel_sample_bytes(out_fmt);
    // conv.rs:516-532 on a sample that is an i16 << 16: the unsigned formats flip the sign bit, every integer format keeps the top bytes
    a.flip = (out_fmt == SYMACCEL_FMT_U8 || out_fmt == SYMACCEL_FMT_U16 || out_fmt == SYMACCEL_FMT_U24 || out_fmt == SYMACCEL_FMT_U32) ? 0x80000000u : 0u;
    a.shr = sb == 0 ? 0u : 32u - 8u * sb;
    a.f32 = out_fmt == SYMACCEL_FMT_F32;  // conv.rs:531: (i16 << 16) / 2^31 = i16 / 2^15, exact in f32
    // ten one-wavefront workgroups per compute unit is what their 15 KiB of LDS lets a compute unit hold
    const dim3 grid((unsigned)std::min<size_t>(a.n_tiles, (size_t)ctx->n_cus * 10));
    switch (codec) {
    case SYMACCEL_ADPCM_MS: adpcm_launch_ch<SYMACCEL_ADPCM_MS>(channels, sb, grid, stream, a); break;
    case SYMACCEL_ADPCM_IMA_WAV: adpcm_launch_ch<SYMACCEL_ADPCM_IMA_WAV>(channels, sb, grid, stream, a); break;
    default: adpcm_launch_ch<SYMACCEL_ADPCM_IMA_QT>(channels, sb, grid, stream, a); break;
    }
    SYM_GPU(ctx, hipGetLastError());
    return SYMACCEL_OK;
}

}  // namespace symaccel
