// PCM and G.711 (symphonia-codec-pcm): packet bytes to PCM, the whole of PcmDecoder::decode_inner on the device.
//
//   lib.rs:50-84     read_pcm_signed / read_pcm_unsigned: plane[idx] = (read << shift).into_sample(), channel after channel of a frame
//   lib.rs:86-118    read_pcm_floating / read_pcm_transfer_func: the bytes reinterpreted; alaw_to_linear / mulaw_to_linear into an i16
//   lib.rs:154-181   the two G.711 expansions
//   lib.rs:336-360   the 24-bit reads are read_[be_]{i,u}24() << 8: left-justified in 32 bits, shifted there, and brought back by
//                    i24::from(x >> 8) / u24::from(x >> 8) (conv.rs:528, 583), whose clamp (sample.rs:272-276, 457-461) then has nothing to do
//   io/mod.rs:204-234 the 24-bit reads themselves
//
// Nothing is carried from sample to sample, so the unit of work is a sample and a TILE is a range of frames of ONE packet
// (pcm_decode_tile_frames: at most 16 KiB of coded bytes and of output): one packet of millions of frames fills the device as well as
// thousands of small packets do.  A workgroup of 256 lanes takes a tile through three steps:
//
//   load     the aligned 16-byte units that cover the tile's coded bytes, lanes side by side, into an LDS image (image byte b is the byte at
//            (the tile's address rounded down to 16) + b).  A unit that reaches outside the input -- only the first and the last unit of the
//            whole input can -- is loaded bytewise: nothing before the first or behind the last byte of the input is read;
//   decode   lane l takes samples l, l + 256, ... of the tile in coded order (frame i / channels, channel i % channels -- the quotient by a
//            multiplication with a reciprocal the host worked out: an integer division would be the only fused arithmetic of the file),
//            assembles the coded bytes in the codec's byte order, applies the shift or the log expansion and the output conversion
//            (pcm_convert.h), and writes the result into an LDS image of the output as pcm_tile_lds does;
//   store    every output run of the tile -- a plane's frames for the native layout, the interleaved frames for a format -- leaves
//            linearly in aligned 16-byte stores, with bytewise stores for the up to 15 bytes at either end of a run.
//
// A sample is carried left-justified in 32 bits, an unsigned one with its top bit flipped (its i32 twin, conv.rs:589): v << (32 - width +
// shift) drops exactly the bits `<<` drops in the width of the sample type, the native sample is that word shifted back down, and every
// output format is the i32 conversion of it (pcm_convert.h, the note above pcm_from_i8).  F32 / F64 samples are moved as bits: no float
// operation touches them on the native path, and pcm_from_f32 / pcm_from_f64 start from the bits on the others.
//
// The log expansion is the reference's arithmetic (lib.rs:154-181: eight integer operations), not a 256-entry table in LDS: the kernel
// waits for memory either way, the operations hide behind it, and a table would be one more LDS read per sample at an address that
// depends on the data -- up to 64 lanes on one bank -- and one more barrier per workgroup.
//
// No register fast path for the all-aligned shapes: not measured to be faster, so not built.
//
// This file is part of the translation unit of batch_copy.hip (its last lines include it): the list of .hip sources is pinned by
// tests/test_build.py and by the emulation build.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "pcm_convert.h"
#include "symaccel_internal.h"

namespace symaccel {

namespace {

// The source families of the kernel: coded bytes and what is done with them
enum PcmDecSrc { PCMDEC_INT1, PCMDEC_INT2, PCMDEC_INT3, PCMDEC_INT4, PCMDEC_LOG, PCMDEC_F32, PCMDEC_F64 };

__host__ __device__ constexpr unsigned pcmdec_coded(int src) {
    return src == PCMDEC_INT1 || src == PCMDEC_LOG ? 1u : src == PCMDEC_INT2 ? 2u : src == PCMDEC_INT3 ? 3u : src == PCMDEC_F64 ? 8u : 4u;
}
__host__ __device__ constexpr unsigned pcmdec_native(int src) {
    return src == PCMDEC_INT1 ? 1u : (src == PCMDEC_INT2 || src == PCMDEC_LOG) ? 2u : src == PCMDEC_F64 ? 8u : 4u;
}

// the coded bytes, their alignment slack, and the words behind them that pcmdec_ld reads with a sample's last bytes: words no unit wrote
// this tile, whose bits are shifted or masked away and never used
constexpr unsigned kPcmDecInDwords = (kPcmTileBytes + 64) / 4;

struct PcmDecArgs {
    const uint8_t *bytes;
    uint8_t *pcm;
    size_t pitch, n_packets, frames, tiles_per_packet;
    size_t in_total;     // bytes from the first byte of the first packet to the last byte of the last one
    unsigned channels, tile_frames;
    uint32_t recip;      // ceil(2^20 / channels): (i * recip) >> 20 == i / channels for i < 2^14
    uint32_t lsh;        // integer codecs: 32 - 8 * coded bytes + shift
    uint32_t nsh;        // integer codecs: 32 - the format's width
    uint32_t flip;       // 0x80000000 for the unsigned codecs
    uint32_t big_endian;
    uint32_t mulaw;      // PCMDEC_LOG: 0 = A-law
};

// lib.rs:154-167
__device__ __forceinline__ int32_t pcmdec_alaw(uint32_t a) {
    a ^= 0x55u;
    int32_t t = (int32_t)((a & 0x0fu) << 4);
    const uint32_t seg = (a & 0x70u) >> 4;
    if (seg == 0) t += 0x8;
    else if (seg == 1) t += 0x108;
    else t = (t + 0x108) << (seg - 1u);  // (at most 0x1f8 << 6: inside an i16)
    return (a & 0x80u) ? t : -t;
}

// lib.rs:169-181
__device__ __forceinline__ int32_t pcmdec_mulaw(uint32_t mu) {
    mu = ~mu & 0xffu;
    int32_t t = (int32_t)((mu & 0x0fu) << 3) + 0x84;
    t <<= (mu & 0x70u) >> 4;  // (at most 0xfc << 7: inside an i16)
    return (mu & 0x80u) ? 0x84 - t : t - 0x84;
}

// four bytes of the image from byte `off` on (any alignment)
__device__ __forceinline__ uint32_t pcmdec_ld(const uint32_t *img, unsigned off) {
    const uint64_t two = ((uint64_t)img[(off >> 2) + 1] << 32) | img[off >> 2];
    return (uint32_t)(two >> (8u * (off & 3u)));
}

// One output run of a tile: image bytes [at + m, at + m + len) to dst[0, len), where m = the address of dst modulo 16 and `at` is a
// multiple of 16 -- aligned 16-byte stores, the ends bytewise.  All 256 lanes call it.
__device__ __forceinline__ void pcmdec_store_run(const uint32_t *lds, unsigned at, unsigned len, uint8_t *dst) {
    const unsigned tid = threadIdx.x;
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u), end = m + len;
    uint8_t *base = dst - m;                                    // 16-byte aligned
    const unsigned first = (m + 15u) / 16u, last = end / 16u;  // whole 16-byte units [first, last)
    const unsigned d0 = at >> 2;
#pragma clang loop vectorize(disable) interleave(disable)
    for (unsigned u = first + tid; u < last; u += 256u) {
        uint4 v;
        v.x = lds[pcm_lds_dword(d0 + 4u * u)];
        v.y = lds[pcm_lds_dword(d0 + 4u * u + 1)];
        v.z = lds[pcm_lds_dword(d0 + 4u * u + 2)];
        v.w = lds[pcm_lds_dword(d0 + 4u * u + 3)];
        *reinterpret_cast<uint4 *>(base + 16u * (size_t)u) = v;
    }
    const uint8_t *l8 = reinterpret_cast<const uint8_t *>(lds);
    if (first > last) {  // the run lies inside one 16-byte unit
        if (tid < len) dst[tid] = l8[pcm_lds_byte(at + m + tid)];
    } else {
        const unsigned head_end = first * 16u, tail_at = last * 16u;
        if (tid < 16u) {
            if (m + tid < head_end) base[m + tid] = l8[pcm_lds_byte(at + m + tid)];
        } else if (tid < 32u) {
            const unsigned b = tail_at + tid - 16u;
            if (b < end) base[b] = l8[pcm_lds_byte(at + b)];
        }
    }
}

// SRC: PcmDecSrc; DST: 0 = the native planes pcm[packet][channel][frame], else SYMACCEL_FMT_*: pcm[packet][frame][channel]
template <int SRC, int DST>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const PcmDecArgs a) {
    constexpr unsigned CB = pcmdec_coded(SRC), NB = pcmdec_native(SRC), OB = DST == 0 ? NB : pcm_sample_bytes(DST);
    __shared__ alignas(16) uint32_t in_img[kPcmDecInDwords];
    __shared__ uint32_t out_img[kPcmLdsDwords];
    const unsigned tid = threadIdx.x, ch = a.channels, fb = ch * CB;
    const unsigned n_runs = DST == 0 ? ch : 1u;               // output runs of a tile
    const unsigned run_fb = DST == 0 ? NB : ch * OB;          // bytes of a frame in a run
    const unsigned region = (a.tile_frames * run_fb + 31u) & ~15u;  // image bytes of a run: its bytes at any alignment, a multiple of 16
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(a.pcm);

    for (size_t p = blockIdx.y; p < a.n_packets; p += gridDim.y) {
        for (size_t t = blockIdx.x; t < a.tiles_per_packet; t += gridDim.x) {
            const size_t f0 = t * a.tile_frames;
            const unsigned nf = a.frames - f0 < a.tile_frames ? (unsigned)(a.frames - f0) : a.tile_frames;

            // ---- load: the units that cover the tile's coded bytes
            const size_t off = p * a.pitch + f0 * fb;  // of the tile's first byte, from a.bytes
            const unsigned ph = (unsigned)((reinterpret_cast<uintptr_t>(a.bytes) + off) & 15u);
            const unsigned n_units = (ph + nf * fb + 15u) >> 4;
            for (unsigned u = tid; u < n_units; u += 256u) {
                const size_t skip = (size_t)16u * u;  // the unit starts at a.bytes + off - ph + skip
                uint4 v;
                if (off + skip >= ph && off + skip - ph + 16u <= a.in_total) {
                    v = *reinterpret_cast<const uint4 *>(a.bytes + (off + skip - ph));
                } else {  // the first or the last unit of the whole input
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    for (unsigned j = 0; j < 16u; ++j) {
                        const size_t b = off + skip + j;  // byte b - ph of the input
                        if (b >= ph && b - ph < a.in_total) w[j >> 2] |= (uint32_t)a.bytes[b - ph] << (8u * (j & 3u));
                    }
                    v = uint4{w[0], w[1], w[2], w[3]};
                }
                *reinterpret_cast<uint4 *>(in_img + 4u * u) = v;
            }
            __syncthreads();

            // ---- decode
            // where the tile's runs start inside an aligned 16-byte unit: run c is plane c of the packet (native), or the packet's frames
            const size_t run0 = DST == 0 ? (p * ch * a.frames + f0) * NB : (p * a.frames + f0) * run_fb;  // byte offset of run 0 in a.pcm
            const unsigned m0 = (unsigned)((out0 + run0) & 15u), m_step = DST == 0 ? (unsigned)((a.frames * NB) & 15u) : 0u;
            const unsigned ns = nf * ch;
            for (unsigned i = tid; i < ns; i += 256u) {
                const unsigned f = (unsigned)(((uint64_t)i * a.recip) >> 20), c = i - f * ch;
                const unsigned at = ph + i * CB;
                uint32_t lo, hi = 0;  // the coded sample, little-endian
                if constexpr (CB == 1) {
                    lo = (in_img[at >> 2] >> (8u * (at & 3u))) & 0xffu;
                } else if constexpr (CB == 8) {
                    lo = pcmdec_ld(in_img, at);
                    hi = pcmdec_ld(in_img, at + 4u);
                    if (a.big_endian) {
                        const uint32_t x = __builtin_bswap32(lo);
                        lo = __builtin_bswap32(hi);
                        hi = x;
                    }
                } else {
                    lo = pcmdec_ld(in_img, at);
                    if (a.big_endian) lo = __builtin_bswap32(lo << (32u - 8u * CB));
                    else if constexpr (CB != 4) lo &= (1u << (8u * (CB & 3u))) - 1u;
                }
                uint32_t w, w_hi = 0;  // the output sample
                if constexpr (SRC == PCMDEC_F64) {
                    if constexpr (DST == 0) {
                        w = lo;
                        w_hi = hi;
                    } else {
                        w = pcm_from_f64<DST>(((uint64_t)hi << 32) | lo);
                    }
                } else if constexpr (SRC == PCMDEC_F32) {
                    if constexpr (DST == 0) w = lo;
                    else w = pcm_from_f32<DST>(lo);
                } else {
                    uint32_t just;  // left-justified, as an i32
                    if constexpr (SRC == PCMDEC_LOG) just = (uint32_t)(a.mulaw ? pcmdec_mulaw(lo) : pcmdec_alaw(lo)) << 16;
                    else just = (lo << a.lsh) ^ a.flip;
                    if constexpr (DST == 0) w = a.flip ? (just ^ a.flip) >> a.nsh : (uint32_t)((int32_t)just >> a.nsh);
                    else w = pcm_from_i32<DST>(just);
                }
                if constexpr (DST == 0) {
                    const unsigned pos = c * region + ((m0 + c * m_step) & 15u) + f * NB;
                    if constexpr (NB == 8) {
                        pcm_lds_put<4>(out_img, pos, w);
                        pcm_lds_put<4>(out_img, pos + 4u, w_hi);
                    } else {
                        pcm_lds_put<NB>(out_img, pos, w);
                    }
                } else {
                    pcm_lds_put<OB>(out_img, m0 + i * OB, w);
                }
            }
            __syncthreads();

            // ---- store
            for (unsigned r = 0; r < n_runs; ++r)
                pcmdec_store_run(out_img, r * region, nf * run_fb, a.pcm + run0 + (size_t)r * a.frames * NB);
            __syncthreads();  // (the images are reused by the next tile)
        }
    }
}

template <int SRC>
void pcm_decode_launch(int out_fmt, dim3 grid, hipStream_t stream, const PcmDecArgs &a) {
    switch (out_fmt) {
#define SYM_PCMDEC_CASE(F) \
    case F: hipLaunchKernelGGL((pcm_decode_kernel<SRC, F>), grid, dim3(256), 0, stream, a); break;
        SYM_PCMDEC_CASE(0)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_U8)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_S8)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_U16)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_S16)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_U24)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_S24)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_U32)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_S32)
        SYM_PCMDEC_CASE(SYMACCEL_FMT_F32)
#undef SYM_PCMDEC_CASE
    }
}

}  // namespace

// (the caller has checked the shape, the pointers' alignment and the sizes: symaccel_pcm_decode_device)
int launch_pcm_decode(symaccel_ctx *ctx, hipStream_t stream, const void *d_bytes, size_t packet_pitch, size_t n_packets, int codec, unsigned channels,
                      unsigned shift, size_t frames, void *d_pcm, int out_fmt) {
    if (n_packets == 0 || frames == 0) return SYMACCEL_OK;
    const PcmCodec pc = pcm_codec(codec);
    const unsigned out_bytes = out_fmt == 0 ? pc.native : pcm_sample_bytes(out_fmt);
    PcmDecArgs a;
    a.bytes = static_cast<const uint8_t *>(d_bytes);
    a.pcm = static_cast<uint8_t *>(d_pcm);
    a.pitch = packet_pitch;
    a.n_packets = n_packets;
    a.frames = frames;
    a.channels = channels;
    a.tile_frames = pcm_decode_tile_frames(channels, pc.coded, out_bytes);
    a.tiles_per_packet = (frames + a.tile_frames - 1) / a.tile_frames;
    a.in_total = (n_packets - 1) * packet_pitch + frames * channels * pc.coded;
    a.recip = ((1u << 20) + channels - 1u) / channels;
    a.lsh = 32u - 8u * pc.coded + shift;
    a.nsh = 32u - pc.width;
    a.flip = pc.kind == PCM_KIND_UNSIGNED ? 0x80000000u : 0u;
    a.big_endian = pc.big_endian;
    a.mulaw = pc.kind == PCM_KIND_MULAW;
    // four workgroups per compute unit is what their two 16 KiB images let a compute unit hold; more only queue
    const size_t cap = (size_t)ctx->n_cus * 4, gx = std::min(a.tiles_per_packet, cap);
    const dim3 grid((unsigned)gx, (unsigned)std::min<size_t>(n_packets, std::max<size_t>(1, cap / gx)));
    switch (pc.kind) {
    case PCM_KIND_F32: pcm_decode_launch<PCMDEC_F32>(out_fmt, grid, stream, a); break;
    case PCM_KIND_F64: pcm_decode_launch<PCMDEC_F64>(out_fmt, grid, stream, a); break;
    case PCM_KIND_ALAW:
    case PCM_KIND_MULAW: pcm_decode_launch<PCMDEC_LOG>(out_fmt, grid, stream, a); break;
    default:
        if (pc.coded == 1) pcm_decode_launch<PCMDEC_INT1>(out_fmt, grid, stream, a);
        else if (pc.coded == 2) pcm_decode_launch<PCMDEC_INT2>(out_fmt, grid, stream, a);
        else if (pc.coded == 3) pcm_decode_launch<PCMDEC_INT3>(out_fmt, grid, stream, a);
        else pcm_decode_launch<PCMDEC_INT4>(out_fmt, grid, stream, a);
        break;
    }
    SYM_GPU(ctx, hipGetLastError());
    return SYMACCEL_OK;
}

}  // namespace symaccel
