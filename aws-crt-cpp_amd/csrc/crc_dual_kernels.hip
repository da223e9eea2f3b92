// Fused CRC32 + CRC32C scan for gfx950: both checksums from one read of the buffers.
//
// crc32_dual_stream_kernel is crc32_stream_kernel's walk (rows of 512 bytes, lane l owning the 8-byte
// word at 8 l, a three-slot ring of 4 KiB groups in registers) with two braids per lane, one per
// polynomial, advanced from the same payload registers:
//     u_p <- T'^p(u_p ^ lo(w), hi(w)),   T'^p_t[e] = e * x^(8(t+1)) * x^(8*504) mod P_p
//  * The four lookups of hi(w) are indexed by payload bytes only, so both polynomials use the same
//    index: their tables are stored as 8-byte pairs (CRC32 entry, CRC32C entry) and read with one
//    ds_read_b64.  The four lookups of lo(w) are indexed by u_p ^ lo(w) and stay per polynomial on
//    ds_read_b32.  12 LDS reads per lane word per row instead of 16.
//  * LDS (144 KiB, one 1024-thread workgroup per CU):
//      [0, 64 KiB)        lo tables: entry e's 256-byte row holds polynomial p at 128 p, table 7 - q
//                         (byte q of lo) at 32 (3 - q), copy c at 4 c
//      [64 KiB, 128 KiB)  hi tables: entry e's 256-byte row holds table 3 - q (byte q of hi) at
//                         64 (3 - q), copy c at 8 c, each an 8-byte pair
//      [128 KiB, 144 KiB) the K images of x^(-64 l), one per polynomial
//    In slot k a lane reads byte q = (k + j) & 3, j = (lane >> 3) & 3, with copy lane & 7: a ds_read_b32
//    half-wave meets 32 distinct banks, a ds_read_b64 half-wave 32 distinct bank pairs
//    (tests/test_dual_model.py).
//  * A buffer's main region is front-padded virtually with zeros to whole tiles of 1 to 256 groups of
//    4 KiB (free for a raw CRC).  Every group is read through a raw buffer resource over its real bytes:
//    in a first tile the lanes in front of the pad's end load zeros, with no branch.  Every tile starts
//    from zero and ends with the wave's XOR of u_p * x^(-64 l) stored, as a pair, to the tile's word of
//    the per-stream workspace: no atomics, no cross-wave state.
// crc32_dual_finish_kernel then joins a buffer's tiles (Horner in x^(8 TILE) per thread, then a tree in
// LDS), enters the seeds and head bytes times x^(8 mainlen), folds the tail bytes and stores the
// complemented pair.  The payload is read from HBM once.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "engine.h"
#include "gf2.h"
#include "crc_device_common.h"

using namespace amdcrc;

namespace {

constexpr uint32_t kDualLoOff = 0;
constexpr uint32_t kDualHiOff = 65536;
constexpr uint32_t kDualKOff = 131072;
constexpr uint32_t kDualLds = kDualKOff + 2 * 8192;
static_assert(kDualLds <= 160 * 1024, "dual scan LDS");
static_assert(kDualLoOff == 0 && kDualHiOff == 0x10000, "DualBraid::init builds these offsets into its v_perm operands");
static_assert(kW8Row * kW8RowsPerGroup == kDualGroupBytes, "ring slot size");

struct DualGroup {
    uint64_t w[kW8RowsPerGroup];
};

// T'_t[e] from the basis of a per-lane table t
__device__ __forceinline__ uint32_t dual_entry(const uint32_t (&bt)[8], uint32_t e) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v ^= ((e >> i) & 1u) ? bt[i] : 0u;
    return v;
}

// Both table regions from a 1024-thread workgroup: thread (e, s) = (tid >> 2, tid & 3) stores table
// 4 + s of both polynomials into entry e's lo row and the pairs of table s into its hi row.
__device__ __forceinline__ void dual_build_tables(char *lds, uint32_t tid) {
    const uint32_t e = tid >> 2, s = tid & 3u;
    uint32_t bt[8];
    basis_w8_lane<kPoly32>(4u + s, bt);
    const uint32_t lo0 = dual_entry(bt, e);
    basis_w8_lane<kPoly32C>(4u + s, bt);
    const uint32_t lo1 = dual_entry(bt, e);
    basis_w8_lane<kPoly32>(s, bt);
    const uint32_t hi0 = dual_entry(bt, e);
    basis_w8_lane<kPoly32C>(s, bt);
    const uint32_t hi1 = dual_entry(bt, e);
    char *lo = lds + kDualLoOff + (e << 8) + (s << 5);
    *(uint4 *)lo = make_uint4(lo0, lo0, lo0, lo0);
    *(uint4 *)(lo + 16) = make_uint4(lo0, lo0, lo0, lo0);
    *(uint4 *)(lo + 128) = make_uint4(lo1, lo1, lo1, lo1);
    *(uint4 *)(lo + 144) = make_uint4(lo1, lo1, lo1, lo1);
    char *hi = lds + kDualHiOff + (e << 8) + (s << 6);
#pragma unroll
    for (int c = 0; c < 4; ++c) *(uint4 *)(hi + 16 * c) = make_uint4(hi0, hi1, hi0, hi1);
}

struct DualBraid {
    const char *L;
    // per lane and slot k: cst = lo row offset | hi row offset << 8 | 1 << 16 (the hi region's 64 KiB), and
    // the v_perm selectors that make a lo address (byte0 <- cst byte 0, byte1 <- byte q of the dword) and
    // a hi address (byte0 <- cst byte 1, byte1 <- byte q, byte2 <- cst byte 2)
    uint32_t cst[4], slo[4], shi[4];
    struct Hi {
        uint64_t v[4];
    };
    __device__ void init(const char *lds, int lane) {
        L = lds;
        const uint32_t j = ((uint32_t)lane >> 3) & 3u, c = (uint32_t)lane & 7u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t q = (k + j) & 3u;
            cst[k] = (((3u - q) << 5) | (c << 2)) | ((((3u - q) << 6) | (c << 3)) << 8) | (kDualHiOff & 0x00ff0000u);
            slo[k] = 0x0c0c0004u | (q << 8);
            shi[k] = 0x0c060005u | (q << 8);
        }
    }
    // the hi dword's four pair lookups (independent of the braids: issued a row ahead)
    __device__ __forceinline__ Hi look_hi(uint32_t hi) const {
        Hi h;
#pragma unroll
        for (int k = 0; k < 4; ++k) h.v[k] = lds64(L, __builtin_amdgcn_perm(cst[k], hi, shi[k]));
        return h;
    }
    // the two chains' lookups of x_p = u_p ^ lo(w), joined with the row's hi pairs and the next row's lo
    __device__ __forceinline__ void look_lo(uint32_t &x0, uint32_t &x1, const Hi &h, uint32_t wn) const {
        uint32_t a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[k] = lds32(L + kDualLoOff, __builtin_amdgcn_perm(cst[k], x0, slo[k]));
            b[k] = lds32(L + kDualLoOff + 128, __builtin_amdgcn_perm(cst[k], x1, slo[k]));
        }
        x0 = xor3(xor3(xor3((uint32_t)h.v[0], (uint32_t)h.v[1], (uint32_t)h.v[2]), (uint32_t)h.v[3], wn), xor3(a[0], a[1], a[2]),
                  a[3]);
        x1 = xor3(xor3(xor3((uint32_t)(h.v[0] >> 32), (uint32_t)(h.v[1] >> 32), (uint32_t)(h.v[2] >> 32)),
                       (uint32_t)(h.v[3] >> 32), wn),
                  xor3(b[0], b[1], b[2]), b[3]);
    }
    // r * x^(-64 lane) for polynomial p: 32 matrix columns of the K image
    __device__ __forceinline__ uint32_t mulK(uint32_t r, int p, int lane) const {
        const char *C = L + kDualKOff + 8192 * p;
        uint32_t acc = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const uint4 c = *(const uint4 *)(C + (g * 64 + lane) * 16);
            acc = xor_and(acc, c.x, (uint32_t)__builtin_amdgcn_sbfe((int)r, 31 - (4 * g + 0), 1));
            acc = xor_and(acc, c.y, (uint32_t)__builtin_amdgcn_sbfe((int)r, 31 - (4 * g + 1), 1));
            acc = xor_and(acc, c.z, (uint32_t)__builtin_amdgcn_sbfe((int)r, 31 - (4 * g + 2), 1));
            acc = xor_and(acc, c.w, (uint32_t)__builtin_amdgcn_sbfe((int)r, 31 - (4 * g + 3), 1));
        }
        return acc;
    }
};

// A group's source: a raw buffer resource over its real bytes (a first tile's group starts `adj`
// bytes late, at the front pad's end: lanes in front of it get offsets past the records and load
// zeros, with no branch and no traffic; a wave's placeholder groups past its last have no records)
struct DualSrc {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t o0, lim;
};
template <int R>
__device__ __forceinline__ void dual_issue(DualGroup &g, const DualSrc &s) {
    if constexpr (R < kW8RowsPerGroup) {
        g.w[R] = bld_w8<R>(s.rs, s.o0, s.lim);
        dual_issue<R + 1>(g, s);
    }
}

// One group: x_p = u_p ^ lo(w_r) are the chained values; the hi pairs of row r are looked up with row
// r - 1's chain step and join at row r; the next-but-one group's row r is issued at row r.
template <int R>
__device__ __forceinline__ void dual_rows(uint32_t &x0, uint32_t &x1, DualBraid::Hi h, const DualGroup &cur, DualGroup &nxt,
                                          const DualSrc &s, const DualBraid &eng) {
    if constexpr (R < kW8RowsPerGroup) {
        nxt.w[R] = bld_w8<R>(s.rs, s.o0, s.lim);
        if constexpr (R == 0) {
            x0 ^= (uint32_t)cur.w[0];
            x1 ^= (uint32_t)cur.w[0];
        } else {
            eng.look_lo(x0, x1, h, (uint32_t)cur.w[R]);
        }
        const DualBraid::Hi hn = eng.look_hi((uint32_t)(cur.w[R] >> 32));
        __builtin_amdgcn_sched_barrier(0);
        dual_rows<R + 1>(x0, x1, hn, cur, nxt, s, eng);
    } else {
        eng.look_lo(x0, x1, h, 0u);
    }
}

__global__ __launch_bounds__(kDualBlock) void crc32_dual_stream_kernel(const DualParams p) {
    __shared__ __attribute__((aligned(16))) char lds[kDualLds];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63;
    const uint64_t gw = rfl64((uint64_t)blockIdx.x * kDualWaves + (tid >> 6));
    const uint64_t t0 = gw * p.split_q + (gw < p.split_r ? gw : (uint64_t)p.split_r);
    const uint64_t ntw = t0 < p.ntiles ? p.split_q + (gw < p.split_r ? 1u : 0u) : 0u;
    const uint32_t G = p.groups_per_tile;
    const uint64_t T = p.tiles_per_buf, tile_bytes = (uint64_t)G * kDualGroupBytes;
    const uint32_t nq = (uint32_t)(ntw * G);  // groups of this wave
    const uint32_t voff = 8u * (uint32_t)lane;
    const uint64_t dummy = (uint64_t)p.d_k[0];

    // prefetch cursor: buffer fb, tile fk of it, group fg of the tile; fmain = the buffer's main region
    uint64_t fb = rfl64(ntw ? t0 / T : 0), fk = t0 - fb * T;  // (the quotient comes from vector code: back to SGPRs)
    uint32_t fg = 0, fq = 0;
    uint64_t fmain = p.base + fb * p.stride + p.hoff;
    auto f_src = [&]() -> DualSrc {
        // virtual offset of the group in the padded main region; the pad lies in tile 0 only
        const uint64_t v = fk * tile_bytes + (uint64_t)fg * kDualGroupBytes;
        const uint32_t adj = v >= p.pad ? 0u : (p.pad - v >= kDualGroupBytes ? (uint32_t)kDualGroupBytes : (uint32_t)(p.pad - v));
        const bool real = fq < nq;
        const uint32_t rec = real ? (uint32_t)kDualGroupBytes - adj : 0u;
        DualSrc s;
        s.rs = list_rsrc(real ? fmain + v - p.pad + adj : dummy, rec);
        s.o0 = real ? voff - adj : voff;
        s.lim = rec;
        return s;
    };
    auto f_next = [&]() {
        if (++fq >= nq) return;
        if (++fg == G) {
            fg = 0;
            if (++fk == T) fk = 0, ++fb, fmain += p.stride;
        }
    };
    // the K images: 512 chunks of 16 bytes per polynomial (loaded first: waiting for them then leaves the
    // ring's loads in flight)
    const uint32_t *kimg = tid < 512u ? p.d_k[0] : p.d_k[1];
    const v4u kq = *(gv4u *)(kimg + 4 * (tid & 511u));
    // the wave's first two groups are in flight while the tables are built
    DualGroup ra, rb, rc;
    dual_issue<0>(ra, f_src());
    f_next();
    dual_issue<0>(rb, f_src());
    f_next();
    dual_build_tables(lds, tid);
    *(v4u *)(lds + kDualKOff + 16 * tid) = kq;
    __syncthreads();
    if (nq == 0) return;  // (its two placeholder groups had no records)
    DualBraid eng;
    eng.init(lds, lane);

    uint64_t st = t0;  // the tile being scanned
    const uint64_t tend = t0 + ntw;
    uint32_t q = 0, g = 0, u0 = 0, u1 = 0;
    auto step = [&](DualGroup &cur, DualGroup &nxt) {
        const DualSrc s = f_src();
        f_next();
        dual_rows<0>(u0, u1, DualBraid::Hi{}, cur, nxt, s, eng);
        ++q;
        if (++g == G) {
            g = 0;
            const uint32_t r0 = wave_xor_s(eng.mulK(u0, 0, lane)), r1 = wave_xor_s(eng.mulK(u1, 1, lane));
            // (inline asm, as the other scans' result stores: a compiler-visible store inside the scan loop
            // makes its wait counts at the loop header pessimistic, and the ring is then drained every step)
            if (lane == 0 && st < tend) {
                const uint2 pr = make_uint2(r0, r1);
                asm volatile("global_store_dwordx2 %0, %1, off" : : "v"(p.d_tiles + 2 * st), "v"(pr) : "memory");
            }
            ++st;
            u0 = u1 = 0;
        }
    };
    // Whole rotations of the ring only, no exit between the steps and none after the loop (a tail of one
    // or two steps made the compiler copy the ring at the loop header, behind a full vmcnt(0) drain in
    // every rotation).  The up to two steps past the wave's last group scan placeholder zeros: the
    // braids are zero after the last tile's finish and stay zero, and nothing is stored past tend.
    while (q < nq) {
        step(ra, rc);
        step(rb, ra);
        step(rc, rb);
    }
}

// ---- the finish pass: one workgroup per buffer
// (a0 * b0 mod P32, a1 * b1 mod P32C): the two polynomials' chains interleaved
__device__ __forceinline__ void dual_mulmod2(uint32_t &a0, uint32_t b0, uint32_t &a1, uint32_t b1) {
    uint32_t r0 = 0, r1 = 0;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) {
        r0 ^= (a0 & (0x80000000u >> i)) ? b0 : 0u;
        r1 ^= (a1 & (0x80000000u >> i)) ? b1 : 0u;
        b0 = (b0 >> 1) ^ ((b0 & 1u) ? kPoly32 : 0u);
        b1 = (b1 >> 1) ^ ((b1 & 1u) ? kPoly32C : 0u);
    }
    a0 = r0;
    a1 = r1;
}
__device__ __forceinline__ uint32_t dual_bytes(uint32_t s, const uint8_t *a, const uint8_t *end, uint32_t poly) {
    for (; a < end; ++a) {
        s ^= *a;
        for (int i = 0; i < 8; ++i) s = (s >> 1) ^ ((s & 1u) ? poly : 0u);
    }
    return s;
}

// The buffer's T tile pairs are the last T of N = per * ne leaves (per and ne powers of two, ne <= the
// workgroup's threads; the leaves in front are zero tiles, free for a raw CRC).  Thread t < ne joins its
// per leaves by Horner in x^(8 TILE); a tree then joins neighbours, left * x^(8 TILE per s) ^ right for
// s = 1, 2, 4, ...: the shifts are DualParams::xlev (x^(8 TILE 2^l), from the host).
__global__ __launch_bounds__(1024) void crc32_dual_finish_kernel(const DualParams p) {
    __shared__ uint32_t v0[1024], v1[1024];
    const uint64_t b = blockIdx.x, T = p.tiles_per_buf;
    const uint32_t tid = threadIdx.x, nth = blockDim.x;
    uint32_t lp = 0;
    while (((uint64_t)nth << lp) < T) ++lp;
    const uint64_t per = 1ull << lp, parts = (T + per - 1) >> lp;
    uint32_t ne = 1;
    while (ne < parts) ne <<= 1;
    const uint64_t zero = per * ne - T;  // zero leaves in front
    uint32_t a0 = 0, a1 = 0;
    if (tid < ne) {
        for (uint64_t j = (uint64_t)tid * per; j < ((uint64_t)tid + 1) * per; ++j) {
            if (j < zero) continue;
            dual_mulmod2(a0, p.xlev[0][0], a1, p.xlev[1][0]);
            const uint2 r = *(const uint2 *)(p.d_tiles + 2 * (b * T + (j - zero)));
            a0 ^= r.x;
            a1 ^= r.y;
        }
    }
    v0[tid] = a0;
    v1[tid] = a1;
    __syncthreads();
    uint32_t lev = lp;
    for (uint32_t s = 1; s < ne; s <<= 1, ++lev) {
        if (tid < ne && (tid & (2 * s - 1)) == 0) {
            uint32_t l0 = v0[tid], l1 = v1[tid];
            dual_mulmod2(l0, p.xlev[0][lev], l1, p.xlev[1][lev]);
            v0[tid] = l0 ^ v0[tid + s];
            v1[tid] = l1 ^ v1[tid + s];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const uint8_t *ptr = (const uint8_t *)(p.base + b * p.stride);
    uint32_t s0 = ~(p.d_seeds ? p.d_seeds[2 * b] : 0u), s1 = ~(p.d_seeds ? p.d_seeds[2 * b + 1] : 0u);
    s0 = dual_bytes(s0, ptr, ptr + p.hoff, kPoly32);
    s1 = dual_bytes(s1, ptr, ptr + p.hoff, kPoly32C);
    dual_mulmod2(s0, p.xmain[0], s1, p.xmain[1]);
    s0 ^= v0[0];
    s1 ^= v1[0];
    s0 = dual_bytes(s0, ptr + p.hoff + p.mainlen, ptr + p.len, kPoly32);
    s1 = dual_bytes(s1, ptr + p.hoff + p.mainlen, ptr + p.len, kPoly32C);
    p.d_out[2 * b] = ~s0;
    p.d_out[2 * b + 1] = ~s1;
}

// ---- buffers without a whole tile: the two single scans run on split seeds, their results are paired
__global__ __launch_bounds__(256) void dual_split_kernel(const uint32_t *pairs, uint32_t *a, uint32_t *b, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = pairs[2 * i], b[i] = pairs[2 * i + 1];
}
__global__ __launch_bounds__(256) void dual_join_kernel(const uint32_t *a, const uint32_t *b, uint32_t *pairs, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) pairs[2 * i] = a[i], pairs[2 * i + 1] = b[i];
}

}  // namespace

// ev[0] / ev[1] (may be null): HIP events stamped with the scan's start and the finish pass's end
extern "C" int amdcrc_launch_dual(const DualParams *p, int nblocks, int finish_threads, void *stream, void *const *ev) {
    hipStream_t s = (hipStream_t)stream;
    if (ev && ev[0])
        hipExtLaunchKernelGGL(crc32_dual_stream_kernel, dim3(nblocks), dim3(kDualBlock), 0, s, (hipEvent_t)ev[0], nullptr, 0, *p);
    else
        hipLaunchKernelGGL(crc32_dual_stream_kernel, dim3(nblocks), dim3(kDualBlock), 0, s, *p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (ev && ev[1])
        hipExtLaunchKernelGGL(crc32_dual_finish_kernel, dim3((unsigned)p->count), dim3(finish_threads), 0, s, nullptr,
                              (hipEvent_t)ev[1], 0, *p);
    else
        hipLaunchKernelGGL(crc32_dual_finish_kernel, dim3((unsigned)p->count), dim3(finish_threads), 0, s, *p);
    return (int)hipGetLastError();
}

extern "C" int amdcrc_launch_dual_split(const uint32_t *d_pairs, uint32_t *d_a, uint32_t *d_b, uint64_t n, void *stream) {
    hipLaunchKernelGGL(dual_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_pairs, d_a, d_b, n);
    return (int)hipGetLastError();
}
extern "C" int amdcrc_launch_dual_join(const uint32_t *d_a, const uint32_t *d_b, uint32_t *d_pairs, uint64_t n, void *stream) {
    hipLaunchKernelGGL(dual_join_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_a, d_b, d_pairs, n);
    return (int)hipGetLastError();
}
