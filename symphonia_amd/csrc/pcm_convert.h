// PCM delivery in the caller's sample format: the reference's FromSample conversions (symphonia-core/src/audio/conv.rs:521-532 for an
// i32 source, 596-607 for an f32 source, clamp_f32 of util.rs:258-266) and the interleaving of audio/util.rs:119-167, as device functions.
//
// Sources are the two forms the library leaves PCM in: F32 planes (the transform codecs) and S32 planes (FLAC / ALAC, left-justified).
// A converted sample is carried as the low `bytes` bytes of a 32-bit word; 24-bit samples are three packed little-endian bytes
// (sample.rs: to_ne_sample_bytes of i24 / u24 on a little-endian host).
//
// Two tile routines turn a frame range of one interleave group into its contiguous output bytes:
//   pcm_tile_regs   mono / stereo into 1-, 2- and 4-byte samples, everything 16-byte aligned: 16-byte loads along each plane, the
//                   samples of a lane packed in registers, 16-byte stores;
//   pcm_tile_lds    everything else (3..8 channels, the 3-byte formats, ragged ends, unaligned planes or output): 16-byte loads along
//                   each plane, the converted samples written to their interleaved place in an LDS image of the output, which is then
//                   written out linearly, 16 bytes per lane.
// Arithmetic contract: float operations are the reference's, one rounding each (the build never contracts: -ffp-contract=off); a float
// to integer cast truncates toward zero, saturates, and maps NaN to 0, as Rust's `as` does.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "symaccel_internal.h"

namespace symaccel {

__host__ __device__ constexpr unsigned pcm_sample_bytes(int fmt) {
    return fmt == SYMACCEL_FMT_U8 || fmt == SYMACCEL_FMT_S8     ? 1u
           : fmt == SYMACCEL_FMT_U16 || fmt == SYMACCEL_FMT_S16 ? 2u
           : fmt == SYMACCEL_FMT_U24 || fmt == SYMACCEL_FMT_S24 ? 3u
           : fmt == SYMACCEL_FMT_U32 || fmt == SYMACCEL_FMT_S32 || fmt == SYMACCEL_FMT_F32 ? 4u
                                                                                             : 0u;
}

// ---- the 18 conversions ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float pcm_bits_f32(uint32_t b) { return __uint_as_float(b); }

// util.rs:258-266 (a NaN fails both comparisons and passes)
__device__ __forceinline__ float pcm_clamp_f32(float v) {
    float c = v;
    c = c > 1.0f ? 1.0f : c;
    c = c < -1.0f ? -1.0f : c;
    return c;
}

// Rust's `x as uN` for x >= 0 or NaN in the ranges that occur here (x <= 2^N): truncation, saturation at 2^N - 1, NaN -> 0
__device__ __forceinline__ uint32_t pcm_f32_as_unsigned(float x, float two_n, uint32_t max) {
    if (!(x > 0.0f)) return 0u;  // (-0, 0, NaN; negative values do not occur behind `clamped() + 1.0`)
    return x >= two_n ? max : (uint32_t)x;
}

// Rust's `x as iN` for |x| <= 2^(N-1) or NaN
__device__ __forceinline__ int32_t pcm_f32_as_signed(float x, float two_n1, int32_t max) {
    if (x != x) return 0;
    return x >= two_n1 ? max : (int32_t)x;  // (x >= -2^(N-1): the cast is exact at the lower end)
}

// (x + 1.0) * 2^k of conv.rs:596-598: the sum rounded to f32, then the scaling.  The scaling by a power of two is exact, and it is written
// as one (ldexp) so that the pair cannot be rewritten into a fused multiply-add of x, 2^k and 2^k -- which would round the same here, but
// no kernel of this library holds a fused f32 operation (tests/test_build.py)
__device__ __forceinline__ float pcm_unsigned_scale(float c, int k) { return __builtin_ldexpf(c + 1.0f, k); }

template <int DST>
__device__ __forceinline__ uint32_t pcm_from_f32(uint32_t bits) {
    if constexpr (DST == SYMACCEL_FMT_F32) {
        return bits;  // conv.rs:606
    } else {
        const float c = pcm_clamp_f32(pcm_bits_f32(bits));
        if constexpr (DST == SYMACCEL_FMT_U8) {
            return pcm_f32_as_unsigned(pcm_unsigned_scale(c, 7), 256.0f, 0xffu);  // conv.rs:596
        } else if constexpr (DST == SYMACCEL_FMT_U16) {
            return pcm_f32_as_unsigned(pcm_unsigned_scale(c, 15), 65536.0f, 0xffffu);  // conv.rs:597
        } else if constexpr (DST == SYMACCEL_FMT_U24) {
            return pcm_f32_as_unsigned(pcm_unsigned_scale(c, 23), 16777216.0f, 0xffffffu);  // conv.rs:598 (u24::from clamps: sample.rs:457-461)
        } else if constexpr (DST == SYMACCEL_FMT_U32) {
            const double x = (double)(c + 1.0f) * 2147483648.0;  // conv.rs:599
            if (!(x > 0.0)) return 0u;
            return x >= 4294967296.0 ? 0xffffffffu : (uint32_t)x;
        } else if constexpr (DST == SYMACCEL_FMT_S8) {
            return (uint32_t)pcm_f32_as_signed(c * 128.0f, 128.0f, 0x7f) & 0xffu;  // conv.rs:601
        } else if constexpr (DST == SYMACCEL_FMT_S16) {
            return (uint32_t)pcm_f32_as_signed(c * 32768.0f, 32768.0f, 0x7fff) & 0xffffu;  // conv.rs:602
        } else if constexpr (DST == SYMACCEL_FMT_S24) {
            return (uint32_t)pcm_f32_as_signed(c * 8388608.0f, 8388608.0f, 0x7fffff) & 0xffffffu;  // conv.rs:603 (i24::from clamps: sample.rs:272-276)
        } else {
            static_assert(DST == SYMACCEL_FMT_S32, "unknown destination format");
            const double x = (double)c * 2147483648.0;  // conv.rs:604
            if (x != x) return 0u;
            return x >= 2147483648.0 ? 0x7fffffffu : (uint32_t)(int32_t)x;
        }
    }
}

template <int DST>
__device__ __forceinline__ uint32_t pcm_from_i32(uint32_t bits) {
    const uint32_t u = bits + 0x80000000u;  // i32_to_u32, conv.rs:516-519
    const int32_t s = (int32_t)bits;
    if constexpr (DST == SYMACCEL_FMT_U8) return u >> 24;                                // conv.rs:521
    else if constexpr (DST == SYMACCEL_FMT_U16) return u >> 16;                          // conv.rs:522
    else if constexpr (DST == SYMACCEL_FMT_U24) return u >> 8;                           // conv.rs:523
    else if constexpr (DST == SYMACCEL_FMT_U32) return u;                                // conv.rs:524
    else if constexpr (DST == SYMACCEL_FMT_S8) return (uint32_t)(s >> 24) & 0xffu;       // conv.rs:526
    else if constexpr (DST == SYMACCEL_FMT_S16) return (uint32_t)(s >> 16) & 0xffffu;    // conv.rs:527
    else if constexpr (DST == SYMACCEL_FMT_S24) return (uint32_t)(s >> 8) & 0xffffffu;   // conv.rs:528
    else if constexpr (DST == SYMACCEL_FMT_S32) return bits;                             // conv.rs:529
    else {
        static_assert(DST == SYMACCEL_FMT_F32, "unknown destination format");
        return __float_as_uint((float)((double)s / 2147483648.0));  // conv.rs:531
    }
}

// ---- the eight further source types: the buffers symphonia-codec-pcm decodes into (pcm_decode.hip) -----------------------------------
//
// A native sample arrives as Rust holds it: an i8 / i16 sign-extended, an i24 sign-extended and in range (sample.rs:272-276: every i24
// the decoder makes is `i24::from`, clamped), a u8 / u16 / u24 / u32 zero-extended, an f64 as its 64 bits.
//
// Every integer conversion of conv.rs:461-592 is the i32 one (conv.rs:521-532) of the sample left-justified in 32 bits, for an unsigned
// source with the top bit flipped (u32 -> i32 is wrapping_sub(2^31), conv.rs:589):
//   * to an integer both sides keep the top bytes of that word, after the same flip of the top bit (i8_to_u8, i16_to_u16, i24_to_u32,
//     wrapping_sub(0x80..)); `clamped()` changes no value that is in range;
//   * to f32 the narrow sources divide the sample by 2^(width-1) and the unsigned ones then subtract 1.0 (conv.rs:471, 491, 511, 546,
//     561, 576): an integer of at most 24 bits is exact in f32, so is its quotient by a power of two, and (s - 2^(w-1)) / 2^(w-1) has at
//     most 24 significant bits, so the subtraction is exact too -- the value is that of the left-justified word over 2^31, which is what
//     conv.rs:531 rounds (nothing to round here).  u32 (conv.rs:591) is computed in f64, exactly, and rounded once, as conv.rs:531 is.
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_i8(uint32_t s) { return pcm_from_i32<DST>(s << 24); }  // conv.rs:461-471
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_i16(uint32_t s) { return pcm_from_i32<DST>(s << 16); }  // conv.rs:481-491
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_i24(uint32_t s) { return pcm_from_i32<DST>(s << 8); }  // conv.rs:501-511
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_u8(uint32_t s) { return pcm_from_i32<DST>((s << 24) ^ 0x80000000u); }  // conv.rs:536-546
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_u16(uint32_t s) { return pcm_from_i32<DST>((s << 16) ^ 0x80000000u); }  // conv.rs:551-561
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_u24(uint32_t s) { return pcm_from_i32<DST>((s << 8) ^ 0x80000000u); }  // conv.rs:566-576
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_u32(uint32_t s) { return pcm_from_i32<DST>(s ^ 0x80000000u); }  // conv.rs:581-591

// util.rs:270-275 (a NaN fails both comparisons and passes)
__device__ __forceinline__ double pcm_clamp_f64(double v) {
    double c = v;
    c = c > 1.0 ? 1.0 : c;
    c = c < -1.0 ? -1.0 : c;
    return c;
}

// Rust's `x as uN` for x in [0, 2^N] or NaN: truncation, saturation at 2^N - 1, NaN -> 0
__device__ __forceinline__ uint32_t pcm_f64_as_unsigned(double x, double two_n, uint32_t max) {
    if (!(x > 0.0)) return 0u;
    return x >= two_n ? max : (uint32_t)x;
}

// Rust's `x as iN` for |x| <= 2^(N-1) or NaN
__device__ __forceinline__ int32_t pcm_f64_as_signed(double x, double two_n1, int32_t max) {
    if (x != x) return 0;
    return x >= two_n1 ? max : (int32_t)x;
}

// conv.rs:611-621.  The arithmetic is the reference's, in f64, one rounding per operation.
template <int DST>
__device__ __forceinline__ uint32_t pcm_from_f64(uint64_t bits) {
    if constexpr (DST == SYMACCEL_FMT_F32) {
        // conv.rs:621, `s as f32`: round to nearest even.  A NaN keeps its sign and the top 22 bits of its payload and becomes quiet -- what
        // the conversion instructions of the reference's targets and of this device make of it, written out so that it holds everywhere
        if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
            return (uint32_t)(bits >> 32 & 0x80000000u) | 0x7fc00000u | (uint32_t)(bits >> 29 & 0x3fffffu);
        return __float_as_uint((float)__builtin_bit_cast(double, bits));
    } else {
        const double c = pcm_clamp_f64(__builtin_bit_cast(double, bits));
        if constexpr (DST == SYMACCEL_FMT_U8) return pcm_f64_as_unsigned((c + 1.0) * 128.0, 256.0, 0xffu);  // conv.rs:611
        else if constexpr (DST == SYMACCEL_FMT_U16) return pcm_f64_as_unsigned((c + 1.0) * 32768.0, 65536.0, 0xffffu);  // conv.rs:612
        else if constexpr (DST == SYMACCEL_FMT_U24) return pcm_f64_as_unsigned((c + 1.0) * 8388608.0, 16777216.0, 0xffffffu);  // conv.rs:613 (u24::from clamps)
        else if constexpr (DST == SYMACCEL_FMT_U32) return pcm_f64_as_unsigned((c + 1.0) * 2147483648.0, 4294967296.0, 0xffffffffu);  // conv.rs:614
        else if constexpr (DST == SYMACCEL_FMT_S8) return (uint32_t)pcm_f64_as_signed(c * 128.0, 128.0, 0x7f) & 0xffu;  // conv.rs:616
        else if constexpr (DST == SYMACCEL_FMT_S16) return (uint32_t)pcm_f64_as_signed(c * 32768.0, 32768.0, 0x7fff) & 0xffffu;  // conv.rs:617
        else if constexpr (DST == SYMACCEL_FMT_S24) return (uint32_t)pcm_f64_as_signed(c * 8388608.0, 8388608.0, 0x7fffff) & 0xffffffu;  // conv.rs:618
        else {
            static_assert(DST == SYMACCEL_FMT_S32, "unknown destination format");
            return (uint32_t)pcm_f64_as_signed(c * 2147483648.0, 2147483648.0, 0x7fffffff);  // conv.rs:619
        }
    }
}

// SRC: SYMACCEL_FMT_F32 or SYMACCEL_FMT_S32
template <int SRC, int DST>
__device__ __forceinline__ uint32_t pcm_convert_sample(uint32_t bits) {
    if constexpr (SRC == SYMACCEL_FMT_F32) return pcm_from_f32<DST>(bits);
    else return pcm_from_i32<DST>(bits);
}

// ---- tiles -------------------------------------------------------------------------------------------------------------------

// The LDS image of a tile's output: byte b of the image stands for the byte at (16-byte aligned global address) + b, so a tile whose
// output starts `m` bytes past a 16-byte boundary begins at image byte m.  One padding dword behind every 32 keeps the strided
// writes of the interleave (lane to lane 4 * channels * bytes apart) off a common bank.
constexpr unsigned kPcmImageDwords = (kPcmTileBytes + 16) / 4;
constexpr unsigned kPcmLdsDwords = kPcmImageDwords + kPcmImageDwords / 32 + 1;

__device__ __forceinline__ unsigned pcm_lds_dword(unsigned d) { return d + (d >> 5); }
__device__ __forceinline__ unsigned pcm_lds_byte(unsigned b) { return pcm_lds_dword(b >> 2) * 4u + (b & 3u); }

template <unsigned BYTES>
__device__ __forceinline__ void pcm_lds_put(uint32_t *lds, unsigned byte, uint32_t v) {
    uint8_t *l8 = reinterpret_cast<uint8_t *>(lds);
    if constexpr (BYTES == 4) {
        lds[pcm_lds_dword(byte >> 2)] = v;  // (4-byte samples sit on 4-byte boundaries: the entry point asks for it)
    } else if constexpr (BYTES == 2) {
        *reinterpret_cast<uint16_t *>(l8 + pcm_lds_byte(byte)) = (uint16_t)v;
    } else if constexpr (BYTES == 1) {
        l8[pcm_lds_byte(byte)] = (uint8_t)v;
    } else {
        l8[pcm_lds_byte(byte)] = (uint8_t)v;
        l8[pcm_lds_byte(byte + 1)] = (uint8_t)(v >> 8);
        l8[pcm_lds_byte(byte + 2)] = (uint8_t)(v >> 16);
    }
}

// `nf` frames (<= pcm_tile_frames) of `channels` planes, plane c at src + c * plane_stride, to dst[nf][channels] samples of DST.
// All 256 work-items of the workgroup call it; `lds` holds kPcmLdsDwords dwords.  src is 4-byte aligned, dst sample-aligned for the
// 2- and 4-byte formats; nothing else is assumed.  Every global load of the body is an aligned 16-byte load along a plane (up to three
// frames at either end of a plane whose address is not a multiple of 16 are loaded alone); the output leaves in 16-byte stores (up to 15
// bytes at either end of a tile that does not start or end on a 16-byte boundary are stored alone).
template <int SRC, int DST>
__device__ __forceinline__ void pcm_tile_lds(const uint32_t *src, size_t plane_stride, unsigned channels, unsigned nf, uint8_t *dst, uint32_t *lds) {
    constexpr unsigned B = pcm_sample_bytes(DST);
    const unsigned tid = threadIdx.x;
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const unsigned frame_bytes = channels * B;
    for (unsigned c = 0; c < channels; ++c) {
        const uint32_t *p = src + (size_t)c * plane_stride;
        unsigned head = (unsigned)((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / 4u;  // frames in front of the first 16-byte boundary
        if (head > nf) head = nf;
        const unsigned quads = (nf - head) / 4u;
        const uint4 *p4 = reinterpret_cast<const uint4 *>(p + head);
        const unsigned at = m + c * B;
        for (unsigned q = tid; q < quads; q += 256u) {
            const uint4 v = p4[q];
            const unsigned f = head + 4u * q;
            pcm_lds_put<B>(lds, at + f * frame_bytes, pcm_convert_sample<SRC, DST>(v.x));
            pcm_lds_put<B>(lds, at + (f + 1) * frame_bytes, pcm_convert_sample<SRC, DST>(v.y));
            pcm_lds_put<B>(lds, at + (f + 2) * frame_bytes, pcm_convert_sample<SRC, DST>(v.z));
            pcm_lds_put<B>(lds, at + (f + 3) * frame_bytes, pcm_convert_sample<SRC, DST>(v.w));
        }
        // the ragged ends: at most 3 + 3 frames per plane
        const unsigned tail0 = head + 4u * quads;
        if (tid < head) pcm_lds_put<B>(lds, at + tid * frame_bytes, pcm_convert_sample<SRC, DST>(p[tid]));
        else if (tid >= 64u && tid - 64u < nf - tail0) pcm_lds_put<B>(lds, at + (tail0 + tid - 64u) * frame_bytes, pcm_convert_sample<SRC, DST>(p[tail0 + tid - 64u]));
    }
    __syncthreads();
    const unsigned end = m + nf * frame_bytes;  // image bytes [m, end) are the tile
    uint8_t *base = dst - m;                    // 16-byte aligned
    const unsigned first = (m + 15u) / 16u, last = end / 16u;  // whole 16-byte units [first, last)
    // (kept from the loop vectoriser: it turns two rounds of this loop into eight 4-byte stores, lane to lane 16 bytes apart)
#pragma clang loop vectorize(disable) interleave(disable)
    for (unsigned u = first + tid; u < last; u += 256u) {
        uint4 v;
        v.x = lds[pcm_lds_dword(4u * u)];
        v.y = lds[pcm_lds_dword(4u * u + 1)];
        v.z = lds[pcm_lds_dword(4u * u + 2)];
        v.w = lds[pcm_lds_dword(4u * u + 3)];
        *reinterpret_cast<uint4 *>(base + 16u * (size_t)u) = v;
    }
    const uint8_t *l8 = reinterpret_cast<const uint8_t *>(lds);
    if (first > last) {  // the tile lies inside one 16-byte unit
        if (tid < end - m) dst[tid] = l8[pcm_lds_byte(m + tid)];
    } else {
        const unsigned head_end = first * 16u, tail_at = last * 16u;
        if (tid < 16u) {
            if (m + tid < head_end) base[m + tid] = l8[pcm_lds_byte(m + tid)];
        } else if (tid < 32u) {
            const unsigned b = tail_at + tid - 16u;
            if (b < end) base[b] = l8[pcm_lds_byte(b)];
        }
    }
    __syncthreads();  // the image is reused by the next tile
}

__host__ __device__ constexpr unsigned pcm_regs_frames(unsigned channels, unsigned bytes) { return 16u / (channels * bytes) > 4u ? 16u / (channels * bytes) : 4u; }

// Mono and stereo into 1-, 2- and 4-byte samples, register to register: a lane takes R = max(4, 16 / (C * B)) consecutive frames, R / 4
// 16-byte loads per plane, and stores R * C * B / 16 16-byte units.  Needs nf % R == 0, planes and dst 16-byte aligned.
template <int SRC, int DST, unsigned C>
__device__ __forceinline__ void pcm_tile_regs(const uint32_t *src, size_t plane_stride, unsigned nf, uint8_t *dst) {
    constexpr unsigned B = pcm_sample_bytes(DST);
    static_assert(B != 3 && C <= 2, "the 3-byte formats and more than two channels go through pcm_tile_lds");
    constexpr unsigned R = pcm_regs_frames(C, B);                        // frames per lane (a power of two)
    constexpr unsigned Q = R / 4u;                                       // 16-byte loads per plane and lane
    constexpr unsigned W = R * C * B / 4u;                               // output dwords per lane (4 or 8)
    constexpr unsigned PER = 4u / B;                                     // samples per output dword
    for (unsigned u = threadIdx.x; u < nf / R; u += 256u) {
        uint32_t s[C][R];
#pragma unroll
        for (unsigned c = 0; c < C; ++c) {
            const uint4 *p4 = reinterpret_cast<const uint4 *>(src + (size_t)c * plane_stride) + (size_t)u * Q;
#pragma unroll
            for (unsigned q = 0; q < Q; ++q) {
                const uint4 v = p4[q];
                s[c][4 * q] = v.x;
                s[c][4 * q + 1] = v.y;
                s[c][4 * q + 2] = v.z;
                s[c][4 * q + 3] = v.w;
            }
        }
        uint32_t w[W];
#pragma unroll
        for (unsigned k = 0; k < W; ++k) {
            uint32_t word = 0;
#pragma unroll
            for (unsigned j = 0; j < PER; ++j) {
                const unsigned i = k * PER + j;  // sample index in the lane's interleaved run: frame i / C, channel i % C
                word |= pcm_convert_sample<SRC, DST>(s[i % C][i / C]) << (8u * B * j);
            }
            w[k] = word;
        }
        uint4 *o = reinterpret_cast<uint4 *>(dst) + (size_t)u * (W / 4u);
#pragma unroll
        for (unsigned k = 0; k < W / 4u; ++k) o[k] = uint4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
    }
}

// One tile, whichever way fits it (a workgroup-uniform choice, nothing per sample).
template <int SRC, int DST>
__device__ __forceinline__ void pcm_tile(const uint32_t *src, size_t plane_stride, unsigned channels, unsigned nf, uint8_t *dst, uint32_t *lds) {
    constexpr unsigned B = pcm_sample_bytes(DST);
    if constexpr (B != 3) {
        if (channels <= 2) {
            const unsigned r = channels == 1 ? pcm_regs_frames(1, B) : pcm_regs_frames(2, B);
            const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (plane_stride * 4u)) & 15u) == 0;
            if (aligned && (nf & (r - 1u)) == 0) {  // (no division in these kernels: its expansion would be their only fused arithmetic)
                if (channels == 1) pcm_tile_regs<SRC, DST, 1>(src, plane_stride, nf, dst);
                else pcm_tile_regs<SRC, DST, 2>(src, plane_stride, nf, dst);
                return;
            }
        }
    }
    pcm_tile_lds<SRC, DST>(src, plane_stride, channels, nf, dst, lds);
}

}  // namespace symaccel
