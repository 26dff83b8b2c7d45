// Layer I / Layer II dequantisation as the fused form of mpa_polyphase_kernel runs it on load: one lane = one sub-band of one
// channel-packet, its record bytes and the table entries they select held in registers for the packet.
//   Layer I  (layer1/mod.rs:51-60, 156-159):   a = sign_extend(code ^ 1 << (bits - 1), bits);  x = scf * (FACTOR[bits] * (a + 1) as f32)
//   Layer II (layer2/mod.rs:198-213, 341-346): a likewise with the class's sample width;  s = a as f32 / 2^(width - 1);
//                                              x = scf[j / 12] * (c * (s + d))
// Every rounded operation is the reference's, in its order.  The division is by a power of two: 2^-(width - 1) is built from its
// exponent and multiplied, which is the same value exactly (|a| <= 2^15, nothing is subnormal) -- a per-lane divisor would
// otherwise expand into a division sequence with fused operations in it.  A sub-band that is not allocated is the +0.0 the
// reference's sample array starts with.
#pragma once

#include "symaccel_internal.h"

namespace symaccel {

template <int NF>
struct Mpa12Lane {
    static constexpr bool kLayer1 = NF == 12;
    static constexpr int kRecBytes = kLayer1 ? 64 : 128;  // bits[32] scf[32] | qclass[32] scf[3][32]
    unsigned alloc = 0;                                   // Layer I: bits (0, 2..15); Layer II: qclass (0, 1..17)
    unsigned scf[3] = {0, 0, 0};
    float scale[3], mul, add;  // mul: FACTOR[bits] | c;  add: unused | d
    unsigned msb, shift;
    float inv_div;

    __device__ __forceinline__ void load(const uint8_t *__restrict__ rec, int sb) {
        alloc = rec[sb];
        scf[0] = rec[32 + sb];
        if constexpr (!kLayer1) {
            scf[1] = rec[64 + sb];
            scf[2] = rec[96 + sb];
        }
    }
    __device__ __forceinline__ bool out_of_range() const {
        if constexpr (kLayer1) return alloc == 1u || alloc > 15u || scf[0] > 63u;
        return alloc > (unsigned)kMpa12Classes || (scf[0] | scf[1] | scf[2]) > 63u;
    }
    // alloc is in range here (out_of_range() lanes were cleared); the indices are masked all the same
    __device__ __forceinline__ void lookup(const float *__restrict__ tbl) {
        unsigned width;
        if constexpr (kLayer1) {
            width = alloc ? (alloc & 15u) : 2u;
            mul = tbl[MPA12_FACTOR + width];
            add = 0.0f;
            scale[0] = scale[1] = scale[2] = tbl[MPA12_SCF + (scf[0] & 63u)];
        } else {
            const unsigned c = alloc ? (alloc - 1u < (unsigned)kMpa12Classes ? alloc - 1u : 0u) : 0u;
            mul = tbl[MPA12_CLASS + 3 * c];
            add = tbl[MPA12_CLASS + 3 * c + 1];
            width = (unsigned)tbl[MPA12_CLASS + 3 * c + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k) scale[k] = tbl[MPA12_SCF + (scf[k] & 63u)];
        }
        msb = 1u << (width - 1u);
        shift = 32u - width;
        inv_div = __uint_as_float((128u - width) << 23);  // 2^-(width - 1)
    }
    // sample j of the sub-band (a compile-time index after unrolling); the code is masked to the width
    __device__ __forceinline__ float dequant(unsigned code, int j) const {
        const unsigned inv = (code & (2u * msb - 1u)) ^ msb;
        const int a = (int)(inv << shift) >> shift;
        float x;
        if constexpr (kLayer1) {
            const float sample = mul * (float)(a + 1);
            x = scale[0] * sample;
        } else {
            const float s = (float)a * inv_div;
            const float t = mul * (s + add);
            x = scale[j / 12] * t;
        }
        return alloc ? x : 0.0f;
    }
};

}  // namespace symaccel
