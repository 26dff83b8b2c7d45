// Gather / scatter between page-locked HOST memory and HBM for the cross-stream batcher (csrc/batcher.cpp): ONE launch moves
// every piece of a chunk -- the submissions of many streams sit in separate page-locked slots, and a hipMemcpyAsync per plane and
// submission (five per submission) costs more host time than the bytes cost link time.  hipHostMalloc memory is mapped into the
// device's address space, so the kernel reads (gather) or writes (scatter) the slots directly; the descriptor list itself is read
// from page-locked memory too.  A workgroup takes one piece of at most 16 KiB: four 16-byte loads per lane in flight, then the
// stores -- with a grid of thousands of pieces the link sees enough outstanding reads to run at its rate.
// Two launches do more than copy: the scatter of a chunk with tickets that want their PCM in a sample format converts and interleaves
// (batch_scatter_convert_kernel), the gather of a chunk with tickets whose FLAC / ALAC words came as int16_t, or row by row as int16_t
// or packed 24-bit words, widens them (batch_gather_widen_kernel); every other chunk is moved by batch_copy_kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "pcm_convert.h"
#include "symaccel_internal.h"

namespace symaccel {

namespace {

// one piece, by the 256 work-items of a workgroup
template <bool NT>
__device__ __forceinline__ void batch_copy_piece(const BatchCopyDesc d, const unsigned tid) {
    const uintptr_t s = reinterpret_cast<uintptr_t>(d.src), t = reinterpret_cast<uintptr_t>(d.dst);
    if (((s | t | d.bytes) & 15u) == 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(d.src);
        uint4 *dst = reinterpret_cast<uint4 *>(d.dst);
        const unsigned n = d.bytes / 16u;  // <= 1024
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + 256u * k < n) {
                if constexpr (NT) {
                    const unsigned *p = reinterpret_cast<const unsigned *>(src + tid + 256u * k);
                    v[k] = uint4{__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2), __builtin_nontemporal_load(p + 3)};
                } else {
                    v[k] = src[tid + 256u * k];
                }
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + 256u * k < n) {
                if constexpr (NT) {
                    unsigned *p = reinterpret_cast<unsigned *>(dst + tid + 256u * k);
                    __builtin_nontemporal_store(v[k].x, p);
                    __builtin_nontemporal_store(v[k].y, p + 1);
                    __builtin_nontemporal_store(v[k].z, p + 2);
                    __builtin_nontemporal_store(v[k].w, p + 3);
                } else {
                    dst[tid + 256u * k] = v[k];
                }
            }
    } else if (((s | t | d.bytes) & 3u) == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(d.src);
        uint32_t *dst = reinterpret_cast<uint32_t *>(d.dst);
        for (unsigned i = tid; i < d.bytes / 4u; i += 256u) dst[i] = src[i];
    } else {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(d.src);
        uint8_t *dst = reinterpret_cast<uint8_t *>(d.dst);
        for (unsigned i = tid; i < d.bytes; i += 256u) dst[i] = src[i];
    }
}

// A capped grid walks the piece list: the link needs about a hundred KiB in flight (50 GB/s x 2 us), not the 32 MiB a grid of one
// workgroup per piece keeps resident -- such a grid fills every wave slot of the device with workgroups that wait for PCIe, and the
// scatter and the synthesis kernel of the neighbouring chunk (other streams) queue behind it instead of running beside it.
// (DIR -- 0 = gather, host to device; 1 = scatter -- changes nothing in the code: it names the two directions apart in a kernel trace)
template <bool NT, int DIR>
__global__ __launch_bounds__(256) void batch_copy_kernel(const BatchCopyDesc *__restrict__ descs, unsigned n_pieces) {
  for (unsigned piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
    const BatchCopyDesc d = descs[piece];
    batch_copy_piece<NT>(d, threadIdx.x);
  }
}

// PCM in the caller's sample format (pcm_convert.h): a capped grid walks the tiles of every interleave group -- a tile is a frame range
// of one group whose output is contiguous and at most kPcmTileBytes long.  One instantiation per (source, destination) pair: nothing
// is decided per sample.
struct PcmConvertArgs {
    const uint32_t *src;
    uint8_t *dst;
    size_t plane_stride, n_frames, dst_group_bytes, n_groups, tiles_per_group;
    unsigned channels, tile_frames;
};

template <int SRC, int DST>
__global__ __launch_bounds__(256) void pcm_convert_kernel(const PcmConvertArgs a) {
    __shared__ uint32_t image[kPcmLdsDwords];
    // (blockIdx.y strides over the groups, blockIdx.x over a group's tiles: no division to find a tile's group)
    for (size_t g = blockIdx.y; g < a.n_groups; g += gridDim.y)
        for (size_t tile = blockIdx.x; tile < a.tiles_per_group; tile += gridDim.x) {
            const size_t f0 = tile * a.tile_frames;
            const unsigned nf = a.n_frames - f0 < a.tile_frames ? (unsigned)(a.n_frames - f0) : a.tile_frames;
            pcm_tile<SRC, DST>(a.src + g * a.channels * a.plane_stride + f0, a.plane_stride, a.channels, nf,
                               a.dst + g * a.dst_group_bytes + f0 * a.channels * pcm_sample_bytes(DST), image);
        }
}

template <int SRC>
void pcm_convert_launch(int dst_fmt, dim3 grid, hipStream_t stream, const PcmConvertArgs &a) {
    switch (dst_fmt) {
#define SYM_PCM_CASE(F) \
    case F: hipLaunchKernelGGL((pcm_convert_kernel<SRC, F>), grid, dim3(256), 0, stream, a); break;
        SYM_PCM_CASE(SYMACCEL_FMT_U8)
        SYM_PCM_CASE(SYMACCEL_FMT_S8)
        SYM_PCM_CASE(SYMACCEL_FMT_U16)
        SYM_PCM_CASE(SYMACCEL_FMT_S16)
        SYM_PCM_CASE(SYMACCEL_FMT_U24)
        SYM_PCM_CASE(SYMACCEL_FMT_S24)
        SYM_PCM_CASE(SYMACCEL_FMT_U32)
        SYM_PCM_CASE(SYMACCEL_FMT_S32)
        SYM_PCM_CASE(SYMACCEL_FMT_F32)
#undef SYM_PCM_CASE
    }
}

// The scatter of a chunk that holds converting pieces (BatchCopyDesc::pad != 0: batcher.cpp, tickets with an output format): `src` is
// the first frame of the piece in the first plane of its interleave group -- the other planes follow `plane_stride` samples apart, the
// same for every piece of a launch --, `dst` and `bytes` the piece's contiguous output in the page-locked slot.  Plain pieces are copied
// as batch_copy_kernel copies them.  The choice is per piece, the same for the whole workgroup.
// batch_copy_piece<false> for the kernel below, with its four 16-byte values in named registers: beside the tile routines the compiler
// keeps the `uint4 v[4]` of batch_copy_piece in scratch memory (80 bytes a lane) and waits for every load before the next.  It is a second
// copy of that routine on purpose: rewriting batch_copy_piece itself would change the kernel every chunk WITHOUT a converting piece runs
// (batch_copy_kernel, unchanged to the instruction), for the sake of the chunks with one.  What follows from it: the plain pieces that
// share a chunk with a converting ticket -- state planes, the PCM of tickets without a format -- are copied by this routine, same access
// pattern, and the development knob SYMACCEL_BATCH_COPY_NT (non-temporal accesses) does not reach such chunks.
__device__ __forceinline__ void batch_copy_piece_beside_tiles(const BatchCopyDesc d, const unsigned tid) {
    const uintptr_t s = reinterpret_cast<uintptr_t>(d.src), t = reinterpret_cast<uintptr_t>(d.dst);
    if (((s | t | d.bytes) & 15u) == 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(d.src);
        uint4 *dst = reinterpret_cast<uint4 *>(d.dst);
        const unsigned n = d.bytes / 16u;  // <= 1024
        const bool p0 = tid < n, p1 = tid + 256u < n, p2 = tid + 512u < n, p3 = tid + 768u < n;
        uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
        if (p0) v0 = src[tid];
        if (p1) v1 = src[tid + 256u];
        if (p2) v2 = src[tid + 512u];
        if (p3) v3 = src[tid + 768u];
        if (p0) dst[tid] = v0;
        if (p1) dst[tid + 256u] = v1;
        if (p2) dst[tid + 512u] = v2;
        if (p3) dst[tid + 768u] = v3;
    } else if (((s | t | d.bytes) & 3u) == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(d.src);
        uint32_t *dst = reinterpret_cast<uint32_t *>(d.dst);
        for (unsigned i = tid; i < d.bytes / 4u; i += 256u) dst[i] = src[i];
    } else {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(d.src);
        uint8_t *dst = reinterpret_cast<uint8_t *>(d.dst);
        for (unsigned i = tid; i < d.bytes; i += 256u) dst[i] = src[i];
    }
}

template <int SRC>
__device__ __forceinline__ void batch_convert_piece(const BatchCopyDesc d, size_t plane_stride, uint32_t *image) {
    const unsigned channels = (d.pad >> 8) & 15u, dst_fmt = d.pad & 15u, frames = (d.pad >> 12) & 0x1fffu;
    const uint32_t *src = static_cast<const uint32_t *>(d.src);
    uint8_t *dst = static_cast<uint8_t *>(d.dst);
    switch (dst_fmt) {
#define SYM_PCM_CASE(F) \
    case F: pcm_tile_lds<SRC, F>(src, plane_stride, channels, frames, dst, image); break;
        SYM_PCM_CASE(SYMACCEL_FMT_U8)
        SYM_PCM_CASE(SYMACCEL_FMT_S8)
        SYM_PCM_CASE(SYMACCEL_FMT_U16)
        SYM_PCM_CASE(SYMACCEL_FMT_S16)
        SYM_PCM_CASE(SYMACCEL_FMT_U24)
        SYM_PCM_CASE(SYMACCEL_FMT_S24)
        SYM_PCM_CASE(SYMACCEL_FMT_U32)
        SYM_PCM_CASE(SYMACCEL_FMT_S32)
        SYM_PCM_CASE(SYMACCEL_FMT_F32)
#undef SYM_PCM_CASE
    }
}

__global__ __launch_bounds__(256) void batch_scatter_convert_kernel(const BatchCopyDesc *__restrict__ descs, unsigned n_pieces, size_t plane_stride) {
    __shared__ uint32_t image[kPcmLdsDwords];
    for (unsigned piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
        const BatchCopyDesc d = descs[piece];
        if (d.pad == 0) batch_copy_piece_beside_tiles(d, threadIdx.x);
        else if (d.pad & kBatchPieceFromI32) batch_convert_piece<SYMACCEL_FMT_S32>(d, plane_stride, image);
        else batch_convert_piece<SYMACCEL_FMT_F32>(d, plane_stride, image);
    }
}

// The gather of a chunk that holds WIDENING pieces (BatchCopyDesc::pad & kBatchPieceWiden: batcher.cpp, tickets whose plane 0 came as
// int16_t -- symaccel_batcher_reserve_io): the mirror image of the converting scatter.  `src` = int16_t words in the page-locked slot (a
// row of odd length starts at a 2-byte boundary), `dst` = int32_t words in HBM, `bytes` = the DESTINATION's (<= kBatchCopyPiece: 4096
// words, 8 KiB of source).  The source is cut at its 16-byte boundaries: up to 7 words of a ragged head, a body of 16-byte loads (8
// words each: at most 512, two per lane), up to 7 words of a ragged tail; every load of a lane -- two of the body, one of the head or
// the tail -- is issued before its first store.  A body load becomes two 16-byte stores where the destination behind the head is 16-byte
// aligned, eight 4-byte stores where it is not.  Nothing outside [src, src + bytes / 2) is read, nothing outside [dst, dst + bytes) written.
// (a compiler vector, not HIP's int4: an int4 built from components is stored word by word, this is ONE 16-byte store)
typedef int widen_v4i __attribute__((vector_size(16)));
__device__ __forceinline__ void widen_store(int32_t *out, const uint4 v, const bool aligned) {
    const int w0 = (int)(v.x << 16) >> 16, w1 = (int)v.x >> 16, w2 = (int)(v.y << 16) >> 16, w3 = (int)v.y >> 16;
    const int w4 = (int)(v.z << 16) >> 16, w5 = (int)v.z >> 16, w6 = (int)(v.w << 16) >> 16, w7 = (int)v.w >> 16;
    if (aligned) {
        widen_v4i *o = reinterpret_cast<widen_v4i *>(out);
        o[0] = widen_v4i{w0, w1, w2, w3};
        o[1] = widen_v4i{w4, w5, w6, w7};
    } else {
        out[0] = w0, out[1] = w1, out[2] = w2, out[3] = w3;
        out[4] = w4, out[5] = w5, out[6] = w6, out[7] = w7;
    }
}

__device__ __forceinline__ void batch_widen_piece(const BatchCopyDesc d, const unsigned tid) {
    const int16_t *src = static_cast<const int16_t *>(d.src);
    int32_t *dst = static_cast<int32_t *>(d.dst);
    const unsigned n = d.bytes / 4u;  // words, <= 4096
    const unsigned to_boundary = (unsigned)((0u - reinterpret_cast<uintptr_t>(src)) & 15u) / 2u;
    const unsigned head = to_boundary < n ? to_boundary : n;
    const unsigned nb = (n - head) / 8u, tail0 = head + 8u * nb;  // nb <= 512
    const uint4 *body = reinterpret_cast<const uint4 *>(src + head);
    int32_t *out = dst + head;
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const bool p0 = tid < nb, p1 = tid + 256u < nb;
    // the ragged ends: lanes 0..7 take the head's words, lanes 8..15 the tail's
    const unsigned r = tid < 8u ? tid : tail0 + (tid - 8u);
    const bool pr = tid < 8u ? tid < head : (tid < 16u && r < n);
    uint4 v0 = {}, v1 = {};
    int16_t e = 0;
    if (p0) v0 = body[tid];
    if (p1) v1 = body[tid + 256u];
    if (pr) e = src[r];
    if (p0) widen_store(out + 8u * tid, v0, aligned);
    if (p1) widen_store(out + 8u * (tid + 256u), v1, aligned);
    if (pr) dst[r] = e;
}

// A PACKED-24 piece (kBatchPieceWiden | kBatchPiecePacked24: a row of a ticket with a width per row, SYMACCEL_IN_FMT_ROWS, sent at 3 bytes a
// word): `src` = little-endian two's-complement 24-bit words, packed, starting 4-byte aligned; `dst` and `bytes` as above (4096 words are
// 12 288 bytes of source).  16 words are 48 bytes, three 16-byte units in and four out, and the source is cut where a 16-byte boundary is a
// word boundary too: a start at 4, 8 or 12 modulo 16 is 4, 8 or 12 words (12, 24, 36 bytes) short of one -- the ragged head --, the body is
// at most 256 groups of 16 words, one per lane, the tail at most 15 words.  Head and tail go byte by byte on lanes 0..11 and 12..26.
// The body crosses the link in the plain copy's pattern -- lane to lane 16 bytes apart, three loads a lane, all issued before anything
// else -- and is dealt out through LDS (12 KiB), so that no load instruction of a wavefront touches a 64-byte line of page-locked memory
// for 16 bytes of it (a lane that loads its own 48 bytes straight from the slot does, in all three loads).  Measured, the two forms run
// the same: 24-bit rows 8 to 10 % BELOW the wide transport at 3/4 of its bytes either way (profiles/flac_row_input*.txt) --
// what packed rows lose is not in how the source is read.  Nothing outside [src, src + 3 * bytes / 4) is read, nothing outside
// [dst, dst + bytes) written.
// (four words out of three dwords: bytes 0-2 | 3-5 | 6-8 | 9-11, each shifted to the top and brought down with its sign)
__device__ __forceinline__ void widen24_store(int32_t *out, const unsigned x, const unsigned y, const unsigned z, const bool aligned) {
    const int w0 = (int)(x << 8) >> 8, w1 = (int)(((x >> 24) | (y << 8)) << 8) >> 8;
    const int w2 = (int)(((y >> 16) | (z << 16)) << 8) >> 8, w3 = (int)z >> 8;
    if (aligned) *reinterpret_cast<widen_v4i *>(out) = widen_v4i{w0, w1, w2, w3};
    else out[0] = w0, out[1] = w1, out[2] = w2, out[3] = w3;
}

constexpr unsigned kWiden24Units = 768;  // 16-byte units of a piece's body at most: 256 groups of three

// (every work-item of the workgroup calls it with the same piece: two barriers inside)
__device__ __forceinline__ void batch_widen24_piece(const BatchCopyDesc d, const unsigned tid, uint4 *image) {
    const uint8_t *src = static_cast<const uint8_t *>(d.src);
    int32_t *dst = static_cast<int32_t *>(d.dst);
    const unsigned n = d.bytes / 4u;  // words, <= 4096
    const unsigned to_boundary = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u);  // in WORDS: (s + 3 s) % 16 == 0 for s = 0, 4, 8, 12
    const unsigned head = to_boundary < n ? to_boundary : n;
    const unsigned ng = (n - head) / 16u, tail0 = head + 16u * ng;  // ng <= 256
    const unsigned nu = 3u * ng;                                    // <= kWiden24Units
    const uint4 *body = reinterpret_cast<const uint4 *>(src + 3u * head);
    int32_t *out = dst + head;
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const bool p0 = tid < nu, p1 = tid + 256u < nu, p2 = tid + 512u < nu;
    // the ragged ends: lanes 0..11 take the head's words, lanes 12..26 the tail's
    const unsigned r = tid < 12u ? tid : tail0 + (tid - 12u);
    const bool pr = tid < 12u ? tid < head : (tid < 27u && r < n);
    uint4 v0 = {}, v1 = {}, v2 = {};
    unsigned e0 = 0, e1 = 0, e2 = 0;
    if (p0) v0 = body[tid];
    if (p1) v1 = body[tid + 256u];
    if (p2) v2 = body[tid + 512u];
    if (pr) e0 = src[3u * r], e1 = src[3u * r + 1u], e2 = src[3u * r + 2u];
    if (p0) image[tid] = v0;
    if (p1) image[tid + 256u] = v1;
    if (p2) image[tid + 512u] = v2;
    __syncthreads();
    if (tid < ng) {
        const uint4 a = image[3u * tid], b = image[3u * tid + 1u], c = image[3u * tid + 2u];
        int32_t *o = out + 16u * tid;
        widen24_store(o, a.x, a.y, a.z, aligned);
        widen24_store(o + 4, a.w, b.x, b.y, aligned);
        widen24_store(o + 8, b.z, b.w, c.x, aligned);
        widen24_store(o + 12, c.y, c.z, c.w, aligned);
    }
    if (pr) dst[r] = (int)((e0 | (e1 << 8) | (e2 << 16)) << 8) >> 8;
    __syncthreads();  // (the image is the next packed piece's)
}

// (plain pieces -- descriptors, coefficients, state, the rows that came at 4 bytes a word -- as batch_scatter_convert_kernel copies its own)
__global__ __launch_bounds__(256) void batch_gather_widen_kernel(const BatchCopyDesc *__restrict__ descs, unsigned n_pieces) {
    __shared__ uint4 image[kWiden24Units];
    for (unsigned piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
        const BatchCopyDesc d = descs[piece];
        if (d.pad & kBatchPiecePacked24) batch_widen24_piece(d, threadIdx.x, image);
        else if (d.pad & kBatchPieceWiden) batch_widen_piece(d, threadIdx.x);
        else batch_copy_piece_beside_tiles(d, threadIdx.x);
    }
}

}  // namespace

// (the caller has checked formats, channel count, alignment and sizes: symaccel_pcm_convert_device)
int launch_pcm_convert(symaccel_ctx *ctx, hipStream_t stream, const void *d_src, int src_fmt, size_t plane_stride, size_t n_groups, size_t channels,
                       size_t n_frames, void *d_dst, int dst_fmt, size_t dst_group_bytes) {
    if (n_groups == 0 || n_frames == 0) return SYMACCEL_OK;
    PcmConvertArgs a;
    a.src = static_cast<const uint32_t *>(d_src);
    a.dst = static_cast<uint8_t *>(d_dst);
    a.plane_stride = plane_stride;
    a.n_frames = n_frames;
    a.dst_group_bytes = dst_group_bytes;
    a.channels = (unsigned)channels;
    a.tile_frames = pcm_tile_frames((unsigned)channels, pcm_sample_bytes(dst_fmt));
    a.n_groups = n_groups;
    a.tiles_per_group = (n_frames + a.tile_frames - 1) / a.tile_frames;
    // eight workgroups per compute unit keep every wave slot a 256-lane workgroup with a 16 KiB image can have busy; more only queue
    const size_t cap = (size_t)ctx->n_cus * 8, gx = std::min(a.tiles_per_group, cap);
    const dim3 grid((unsigned)gx, (unsigned)std::min<size_t>(n_groups, std::max<size_t>(1, cap / gx)));
    if (src_fmt == SYMACCEL_FMT_F32) pcm_convert_launch<SYMACCEL_FMT_F32>(dst_fmt, grid, stream, a);
    else pcm_convert_launch<SYMACCEL_FMT_S32>(dst_fmt, grid, stream, a);
    SYM_GPU(ctx, hipGetLastError());
    return SYMACCEL_OK;
}

namespace {

// The completion flag of a launch: ONE 64-bit word in page-locked host memory, written behind the last scatter of the launch (same
// stream: the scatter's stores to host memory are complete when this kernel starts).  Waiters read the word -- no runtime call on the
// wait path, nothing for sixteen caller threads to contend on.  The value only grows (a launch sequence number per block).
__global__ void batch_flag_kernel(unsigned long long *flag, unsigned long long seq) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __atomic_store_n(flag, seq, __ATOMIC_RELAXED);
}

}  // namespace

int launch_batch_flag(symaccel_ctx *ctx, hipStream_t stream, uint64_t *h_flag, uint64_t seq) {
    hipLaunchKernelGGL(batch_flag_kernel, dim3(1), dim3(1), 0, stream, reinterpret_cast<unsigned long long *>(h_flag), (unsigned long long)seq);
    SYM_GPU(ctx, hipGetLastError());
    return SYMACCEL_OK;
}

int launch_batch_copy(symaccel_ctx *ctx, hipStream_t stream, const BatchCopyDesc *descs, size_t n, bool scatter, size_t pcm_plane_stride, bool widening) {
    if (n == 0) return SYMACCEL_OK;
    if (n > 0x7fffffffu) return SYMACCEL_ERR_INVALID_ARG;
    // workgroups per copy launch.  64: the link needs few -- a copy kernel that fills the device keeps the synthesis kernel and the copy of
    // the other direction waiting for compute units (256 -> 64: AAC behind the trait 3.96 -> 4.3-4.45 M packets/s at S = 256, 32 and 96 are
    // both slower; profiles/r06z4_big_groups.jsonl, r06z5_copy_grid.jsonl).  Development knobs: SYMACCEL_BATCH_COPY_WGS (both directions;
    // 0 = one workgroup per piece, as round 5 had it), SYMACCEL_BATCH_COPY_WGS_G / _S (gather / scatter alone)
    static const unsigned caps[2] = {
        [] { const char *e = std::getenv("SYMACCEL_BATCH_COPY_WGS_G"); if (!e) e = std::getenv("SYMACCEL_BATCH_COPY_WGS"); return e ? (unsigned)std::atoi(e) : 64u; }(),
        [] { const char *e = std::getenv("SYMACCEL_BATCH_COPY_WGS_S"); if (!e) e = std::getenv("SYMACCEL_BATCH_COPY_WGS"); return e ? (unsigned)std::atoi(e) : 64u; }()};
    const unsigned cap = caps[scatter ? 1 : 0];
    const unsigned grid = cap ? (unsigned)std::min<size_t>(n, cap) : (unsigned)n;
    static const bool nt = [] {  // development knob: non-temporal accesses
        const char *e = std::getenv("SYMACCEL_BATCH_COPY_NT");
        return e && std::atoi(e) != 0;
    }();
    // (pcm_plane_stride != 0: the list holds converting pieces -- only then; every other launch is the plain kernel, as before)
    // (widening: the list of a gather holds widening pieces -- likewise)
    if (pcm_plane_stride) hipLaunchKernelGGL(batch_scatter_convert_kernel, dim3(grid), dim3(256), 0, stream, descs, (unsigned)n, pcm_plane_stride);
    else if (widening && !scatter) hipLaunchKernelGGL(batch_gather_widen_kernel, dim3(grid), dim3(256), 0, stream, descs, (unsigned)n);
    else if (nt && scatter) hipLaunchKernelGGL((batch_copy_kernel<true, 1>), dim3(grid), dim3(256), 0, stream, descs, (unsigned)n);
    else if (nt) hipLaunchKernelGGL((batch_copy_kernel<true, 0>), dim3(grid), dim3(256), 0, stream, descs, (unsigned)n);
    else if (scatter) hipLaunchKernelGGL((batch_copy_kernel<false, 1>), dim3(grid), dim3(256), 0, stream, descs, (unsigned)n);
    else hipLaunchKernelGGL((batch_copy_kernel<false, 0>), dim3(grid), dim3(256), 0, stream, descs, (unsigned)n);
    SYM_GPU(ctx, hipGetLastError());
    return SYMACCEL_OK;
}

}  // namespace symaccel

// The ADPCM decode kernels and their launcher (a file of their own, compiled as part of this translation unit)
#include "adpcm.hip"

// The PCM / G.711 decode kernels and their launcher (likewise)
#include "pcm_decode.hip"
