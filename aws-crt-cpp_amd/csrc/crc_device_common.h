// Device helpers shared by the scan kernels of crc_kernels.hip and crc_dual_kernels.hip: LDS reads,
// wave-uniform values, three-input bit operations, the wave XOR, and the compile-time GF(2) bases of
// the 8-byte-word row step.  Moved here unchanged from crc_kernels.hip; everything
// has internal linkage (an anonymous namespace per translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "gf2.h"

using namespace amdcrc;

namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const v4u gv4u;
typedef __attribute__((address_space(1))) const uint32_t gu32;
typedef __attribute__((address_space(1))) const uint64_t gu64;

__device__ __forceinline__ uint32_t lds32(const char *L, uint32_t a) { return *(const uint32_t *)(L + a); }
__device__ __forceinline__ uint64_t lds64(const char *L, uint32_t a) { return *(const uint64_t *)(L + a); }

__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t xor_and(uint32_t acc, uint32_t c, uint32_t m) {  // acc ^ (c & m)
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x78" : "=v"(r) : "v"(acc), "v"(c), "v"(m));
    return r;
}

// XOR over the 64 lanes, returned wave-uniform: two quad_perm and two row_ror DPP steps leave each
// 16-lane row's XOR in all its lanes; four readlanes finish in scalar registers.
__device__ __forceinline__ uint32_t wave_xor_s(uint32_t v) {
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);  // row_ror:4
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
    return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) ^ __builtin_amdgcn_readlane((int)v, 16) ^
                      __builtin_amdgcn_readlane((int)v, 32) ^ __builtin_amdgcn_readlane((int)v, 48));
}
__device__ __forceinline__ uint64_t wave_xor64_s(uint64_t v) {
    const uint32_t lo = wave_xor_s((uint32_t)v), hi = wave_xor_s((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

constexpr uint32_t kW8Row = 512;
constexpr int kW8RowsPerGroup = 8;  // 4 KiB per wave per ring slot, as the 4-byte rows

template <uint32_t POLY>
struct BraidW8Basis {
    uint32_t b[9][8];  // b[t][i] = T'_t[1 << i] (t < 8); b[8][i] = T_0[1 << i]
    constexpr BraidW8Basis() : b() {
        const uint64_t skip = gf2_xpow8n(kW8Row - 8, POLY, 32);
        for (int i = 0; i < 8; ++i) {
            for (int t = 0; t < 8; ++t) b[t][i] = (uint32_t)gf2_mulmod(gf2_table_entry(1u << i, t, POLY), skip, POLY, 32);
            b[8][i] = (uint32_t)gf2_table_entry(1u << i, 0, POLY);
        }
    }
};
template <uint32_t POLY, int K>
__device__ __forceinline__ uint32_t basis_w8(uint32_t e) {
    constexpr BraidW8Basis<POLY> B{};
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v ^= ((e >> i) & 1u) ? B.b[K][i] : 0u;
    return v;
}
// bt[i] = T'_t[1 << i] for a per-lane t < 8: one AND-OR per candidate through opaque masks (a select
// chain over constants would become a per-lane load from a constant table, waited for behind the
// payload loads already in flight)
template <uint32_t POLY>
__device__ __forceinline__ void basis_w8_lane(uint32_t t, uint32_t (&bt)[8]) {
    constexpr BraidW8Basis<POLY> B{};
    uint32_t m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        m[k] = t == (uint32_t)k ? ~0u : 0u;
        asm("" : "+v"(m[k]));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) v |= B.b[k][i] & m[k];
        bt[i] = v;
    }
}

// a raw buffer resource over [base, base + nrec) (range-checked: loads past nrec return zero) and a
// row load through it (crc32_list_stream_kernel, crc32_dual_stream_kernel)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t list_rsrc(uint64_t base, uint32_t nrec) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)rfl64(base), (short)0, (int)__builtin_amdgcn_readfirstlane(nrec),
                                             0x00020000);
}

template <int R>
__device__ __forceinline__ uint64_t bld_w8(__amdgpu_buffer_rsrc_t rs, uint32_t o0, uint32_t lim) {
    const uint32_t o = __builtin_elementwise_min(o0 + (uint32_t)(R * kW8Row), lim);
    const v2u v = __builtin_amdgcn_raw_buffer_load_b64(rs, o, 0, 2);  // aux 2: non-temporal
    return ((uint64_t)v.y << 32) | v.x;
}

}  // namespace
