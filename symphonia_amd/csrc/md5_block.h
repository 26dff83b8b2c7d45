// One MD5 block (RFC 1321; symphonia-core/src/checksum/md5.rs:12-170), shared by the host functions symaccel_md5_* (host_tools.cpp)
// and the FLAC verification kernel (flac.hip), so both hash with the same code.
//
// gfx950: F and G are one v_bfi_b32 each, H one v_xor3_b32, the three-way sum one v_add3_u32 with M[k] + K[i] added off the
// dependent chain (the message words are known before the block starts), the rotate one v_alignbit_b32: about four dependent
// instructions per step.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace symaccel {

__host__ __device__ __forceinline__ uint32_t md5_rotl(uint32_t x, int s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, (uint32_t)(32 - s));
#else
    return (x << s) | (x >> (32 - s));
#endif
}

__host__ __device__ __forceinline__ uint32_t md5_f(uint32_t b, uint32_t c, uint32_t d) { return (b & c) | (~b & d); }
__host__ __device__ __forceinline__ uint32_t md5_g(uint32_t b, uint32_t c, uint32_t d) { return (d & b) | (~d & c); }
__host__ __device__ __forceinline__ uint32_t md5_h(uint32_t b, uint32_t c, uint32_t d) { return b ^ c ^ d; }
__host__ __device__ __forceinline__ uint32_t md5_i(uint32_t b, uint32_t c, uint32_t d) { return c ^ (b | ~d); }

#define SYM_MD5_STEP(F, a, b, c, d, mk, s) a = b + md5_rotl(a + F(b, c, d) + (mk), s)

// abcd += the transform of the 16 little-endian message words m (md5.rs:29-170)
__host__ __device__ __forceinline__ void md5_block(uint32_t (&abcd)[4], const uint32_t (&m)[16]) {
    uint32_t a = abcd[0], b = abcd[1], c = abcd[2], d = abcd[3];
    SYM_MD5_STEP(md5_f, a, b, c, d, m[0] + 0xd76aa478u, 7);
    SYM_MD5_STEP(md5_f, d, a, b, c, m[1] + 0xe8c7b756u, 12);
    SYM_MD5_STEP(md5_f, c, d, a, b, m[2] + 0x242070dbu, 17);
    SYM_MD5_STEP(md5_f, b, c, d, a, m[3] + 0xc1bdceeeu, 22);
    SYM_MD5_STEP(md5_f, a, b, c, d, m[4] + 0xf57c0fafu, 7);
    SYM_MD5_STEP(md5_f, d, a, b, c, m[5] + 0x4787c62au, 12);
    SYM_MD5_STEP(md5_f, c, d, a, b, m[6] + 0xa8304613u, 17);
    SYM_MD5_STEP(md5_f, b, c, d, a, m[7] + 0xfd469501u, 22);
    SYM_MD5_STEP(md5_f, a, b, c, d, m[8] + 0x698098d8u, 7);
    SYM_MD5_STEP(md5_f, d, a, b, c, m[9] + 0x8b44f7afu, 12);
    SYM_MD5_STEP(md5_f, c, d, a, b, m[10] + 0xffff5bb1u, 17);
    SYM_MD5_STEP(md5_f, b, c, d, a, m[11] + 0x895cd7beu, 22);
    SYM_MD5_STEP(md5_f, a, b, c, d, m[12] + 0x6b901122u, 7);
    SYM_MD5_STEP(md5_f, d, a, b, c, m[13] + 0xfd987193u, 12);
    SYM_MD5_STEP(md5_f, c, d, a, b, m[14] + 0xa679438eu, 17);
    SYM_MD5_STEP(md5_f, b, c, d, a, m[15] + 0x49b40821u, 22);

    SYM_MD5_STEP(md5_g, a, b, c, d, m[1] + 0xf61e2562u, 5);
    SYM_MD5_STEP(md5_g, d, a, b, c, m[6] + 0xc040b340u, 9);
    SYM_MD5_STEP(md5_g, c, d, a, b, m[11] + 0x265e5a51u, 14);
    SYM_MD5_STEP(md5_g, b, c, d, a, m[0] + 0xe9b6c7aau, 20);
    SYM_MD5_STEP(md5_g, a, b, c, d, m[5] + 0xd62f105du, 5);
    SYM_MD5_STEP(md5_g, d, a, b, c, m[10] + 0x02441453u, 9);
    SYM_MD5_STEP(md5_g, c, d, a, b, m[15] + 0xd8a1e681u, 14);
    SYM_MD5_STEP(md5_g, b, c, d, a, m[4] + 0xe7d3fbc8u, 20);
    SYM_MD5_STEP(md5_g, a, b, c, d, m[9] + 0x21e1cde6u, 5);
    SYM_MD5_STEP(md5_g, d, a, b, c, m[14] + 0xc33707d6u, 9);
    SYM_MD5_STEP(md5_g, c, d, a, b, m[3] + 0xf4d50d87u, 14);
    SYM_MD5_STEP(md5_g, b, c, d, a, m[8] + 0x455a14edu, 20);
    SYM_MD5_STEP(md5_g, a, b, c, d, m[13] + 0xa9e3e905u, 5);
    SYM_MD5_STEP(md5_g, d, a, b, c, m[2] + 0xfcefa3f8u, 9);
    SYM_MD5_STEP(md5_g, c, d, a, b, m[7] + 0x676f02d9u, 14);
    SYM_MD5_STEP(md5_g, b, c, d, a, m[12] + 0x8d2a4c8au, 20);

    SYM_MD5_STEP(md5_h, a, b, c, d, m[5] + 0xfffa3942u, 4);
    SYM_MD5_STEP(md5_h, d, a, b, c, m[8] + 0x8771f681u, 11);
    SYM_MD5_STEP(md5_h, c, d, a, b, m[11] + 0x6d9d6122u, 16);
    SYM_MD5_STEP(md5_h, b, c, d, a, m[14] + 0xfde5380cu, 23);
    SYM_MD5_STEP(md5_h, a, b, c, d, m[1] + 0xa4beea44u, 4);
    SYM_MD5_STEP(md5_h, d, a, b, c, m[4] + 0x4bdecfa9u, 11);
    SYM_MD5_STEP(md5_h, c, d, a, b, m[7] + 0xf6bb4b60u, 16);
    SYM_MD5_STEP(md5_h, b, c, d, a, m[10] + 0xbebfbc70u, 23);
    SYM_MD5_STEP(md5_h, a, b, c, d, m[13] + 0x289b7ec6u, 4);
    SYM_MD5_STEP(md5_h, d, a, b, c, m[0] + 0xeaa127fau, 11);
    SYM_MD5_STEP(md5_h, c, d, a, b, m[3] + 0xd4ef3085u, 16);
    SYM_MD5_STEP(md5_h, b, c, d, a, m[6] + 0x04881d05u, 23);
    SYM_MD5_STEP(md5_h, a, b, c, d, m[9] + 0xd9d4d039u, 4);
    SYM_MD5_STEP(md5_h, d, a, b, c, m[12] + 0xe6db99e5u, 11);
    SYM_MD5_STEP(md5_h, c, d, a, b, m[15] + 0x1fa27cf8u, 16);
    SYM_MD5_STEP(md5_h, b, c, d, a, m[2] + 0xc4ac5665u, 23);

    SYM_MD5_STEP(md5_i, a, b, c, d, m[0] + 0xf4292244u, 6);
    SYM_MD5_STEP(md5_i, d, a, b, c, m[7] + 0x432aff97u, 10);
    SYM_MD5_STEP(md5_i, c, d, a, b, m[14] + 0xab9423a7u, 15);
    SYM_MD5_STEP(md5_i, b, c, d, a, m[5] + 0xfc93a039u, 21);
    SYM_MD5_STEP(md5_i, a, b, c, d, m[12] + 0x655b59c3u, 6);
    SYM_MD5_STEP(md5_i, d, a, b, c, m[3] + 0x8f0ccc92u, 10);
    SYM_MD5_STEP(md5_i, c, d, a, b, m[10] + 0xffeff47du, 15);
    SYM_MD5_STEP(md5_i, b, c, d, a, m[1] + 0x85845dd1u, 21);
    SYM_MD5_STEP(md5_i, a, b, c, d, m[8] + 0x6fa87e4fu, 6);
    SYM_MD5_STEP(md5_i, d, a, b, c, m[15] + 0xfe2ce6e0u, 10);
    SYM_MD5_STEP(md5_i, c, d, a, b, m[6] + 0xa3014314u, 15);
    SYM_MD5_STEP(md5_i, b, c, d, a, m[13] + 0x4e0811a1u, 21);
    SYM_MD5_STEP(md5_i, a, b, c, d, m[4] + 0xf7537e82u, 6);
    SYM_MD5_STEP(md5_i, d, a, b, c, m[11] + 0xbd3af235u, 10);
    SYM_MD5_STEP(md5_i, c, d, a, b, m[2] + 0x2ad7d2bbu, 15);
    SYM_MD5_STEP(md5_i, b, c, d, a, m[9] + 0xeb86d391u, 21);
    abcd[0] += a;
    abcd[1] += b;
    abcd[2] += c;
    abcd[3] += d;
}

#undef SYM_MD5_STEP

}  // namespace symaccel
