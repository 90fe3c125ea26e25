// npj_kernels.hip — K2 build, K3 probe, K9 close_gaps for the no-partition join.
//
// Replaces build()/probe()/close_gaps() of npj.cpp:190-212, 216-364 (scalar
// definition 412-445), 475-514.  One global linear-probing table of
// uint64 (payload << 32 | key), empty = 0, exactly the reference's bucket
// format, so a table built here can be probed by the oracle and vice versa.
// Design (not a translation):
//   * build: one tuple per lane, 64-bit global compare-and-swap against 0; the
//     key/payload columns are read with 16-byte loads.
//   * probe: one tuple per lane per chain, four chains per lane from a 16-byte
//     load, each walking consecutive buckets to the first empty one and
//     reporting every key match (the reference's "refill finished lanes" loop,
//     npj.cpp:251-254, exists because its 16 lanes are all it has; here
//     thousands of resident waves hide the divergence instead).
//   * The load factor is a free knob (results do not depend on it): the GPU
//     default is 0.5, the reference's 0.90 (npj.cpp:944) gives ~59-bucket walks.
#include "hj_device.hpp"
#include "hj_internal.hpp"
#include "hj_emit.hpp"
#include "hj_lookup.hpp"

__device__ __forceinline__ u64 npj_bucket(uint32_t key, uint32_t factor, u64 buckets)
{
    // h = ((uint64)(uint32)(key*factor) * buckets) >> 32, buckets may exceed 2^32
    const u64 x = (u64)(uint32_t)(key * factor);
    return (u64)(((unsigned __int128)x * buckets) >> 32);
}

__global__ __launch_bounds__(256) void npj_build_kernel(const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ vals, u64 n,
                                                        u64 *table, u64 buckets, uint32_t factor,
                                                        uint32_t *zero_key_flag, uint32_t line_hash)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t key = keys[i];
        if (key == 0) { atomicOr(zero_key_flag, 1u); continue; }   // npj.cpp:583: 0 is "empty"
        const u64 pair = ((u64)vals[i] << 32) | key;
        // line_hash: walks start on a 64-byte line of 8 buckets (see npj_probe_line_kernel)
        u64 h = line_hash ? npj_bucket(key, factor, buckets >> 3) << 3 : npj_bucket(key, factor, buckets);
        for (;;) {
            // skip the buckets that are visibly taken with plain loads (after the first one the line is
            // in L2; a stale "empty" only costs the failed CAS below, a bucket never becomes empty again):
            // every failed CAS is a round trip to the memory side
            while ((uint32_t)table[h] != 0u) { if (++h == buckets) h = 0; }
            // claim the first bucket whose low word is empty (npj.cpp:204-210)
            const u64 old = atomicCAS(&table[h], 0ull, pair);
            if (old == 0ull) break;
            if (++h == buckets) h = 0;
        }
    }
}

int hj_launch_npj_build(const uint32_t *keys, const uint32_t *vals, size_t n, u64 *table,
                        size_t buckets, uint32_t factor, uint32_t *zero_key_flag,
                        int cus, hipStream_t stream, bool line_hash)
{
    if (buckets <= n) return HJGPU_EINVAL;       // a walk must always find an empty bucket
    if (line_hash && (buckets % 8 != 0 || ((uintptr_t)table & 63))) return HJGPU_EINVAL;
    u64 blocks = (n + 255) / 256;
    if (blocks > (u64)cus * 16) blocks = (u64)cus * 16;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(npj_build_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, keys, vals,
                       (u64)n, table, (u64)buckets, factor, zero_key_flag, line_hash ? 1u : 0u);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

constexpr int NPJ_PROBE_BLOCK = 256;
constexpr int NPJ_PROBE_WAVES = NPJ_PROBE_BLOCK / 64;

// What every probe body starts with: the emitter and this wave's cursor, and the probe columns as 16-byte vectors - the columns are
// aligned down to 16 bytes, tuple i of the relation is component gb + i, the vectors [0, nvec) cover [gb, ge).
struct NpjProbeColumns {
    const uint4 *k4, *v4;
    u64 gb, ge, nvec, stride;
};
template <class Em>
__device__ __forceinline__ NpjProbeColumns npj_probe_begin(const NpjProbeArgs &a, Em &em, u64 (&wave_cursor)[NPJ_PROBE_WAVES])
{
    const int wave = threadIdx.x >> 6;
    em.init(a.ok, a.oov, a.oiv, a.block_size, a.block_limit, a.block_counter, a.overflow,
            &wave_cursor[wave]);
    if (hj_lane() == 0) wave_cursor[wave] = HJ_NO_CURSOR;
    const uint32_t a0 = (uint32_t)(((uintptr_t)a.keys >> 2) & 3);
    NpjProbeColumns c;
    c.k4 = reinterpret_cast<const uint4 *>(a.keys - a0);
    c.v4 = reinterpret_cast<const uint4 *>(a.vals - a0);
    c.gb = a0; c.ge = a0 + a.n;
    c.nvec = (c.ge + 3) >> 2;
    c.stride = (u64)gridDim.x * NPJ_PROBE_BLOCK;
    return c;
}

// The bucket / group walk of every join mode but the inner join (npj_probe_kernel below: the same walk as the kernel's own body, whose
// machine code changes when it is an inlined function; folding it in here waits for a measurement against it) on a table with the
// reference's hash (the line walk further below: the library's own tables).
// GROUPED: the walk fetches aligned groups of 4 buckets (32 bytes, two 16-byte loads
// issued together) instead of one bucket per dependent load.  The walk has to reach
// the first EMPTY bucket (every match counts, npj.cpp:426-442), i.e. 2.5 buckets on
// average at load 0.5: with one bucket per load that is 2.5 dependent memory round
// trips per probe; a group resolves most walks in one.  Needs buckets % 4 == 0
// (the library's own tables; any other table takes the bucket-at-a-time path).
// UNIQUE: the reference's _UNIQUE build (npj.cpp:288-290, 436-438): the walk of a probe key ends at its first match.
// MODE (HJ_MODE_*): semi- / anti-join (HJGPU_FLAG_SEMI / _ANTI, npj_exists_kernel) -
// with UNIQUE's walk, ONE row (key, outer_val) per probe tuple that found a match / that reached an empty bucket without one; left outer
// join (HJGPU_FLAG_LEFT_OUTER, npj_outer_kernel) - the inner join's rows (every match, or the first under UNIQUE), then ONE row
// (key, outer_val, HJGPU_NULL_VAL) per probe tuple whose walk found none.
template <bool GROUPED, bool UNIQUE, int MODE>
__device__ __forceinline__ void npj_probe_body(NpjProbeArgs a)
{
    // LEFTISH: the modes that report like the left outer join; KEEPB (right / full outer joins, never UNIQUE: the walk visits every copy of
    // a key): every bucket a probe matches gets its bit in a.bucket_bits - one bucket per build tuple, so bucket-level marks are exact
    // MARKING (HJ_MODE_MARK, the probe of a right semi- / anti-join): the same marks and nothing else - no row, no aggregate
    constexpr bool LEFTISH = MODE == HJ_MODE_LEFT_OUTER || MODE == HJ_MODE_FULL_OUTER;
    constexpr bool MARKING = MODE == HJ_MODE_MARK;
    constexpr bool MATCHES = LEFTISH || MODE == HJ_MODE_RIGHT_OUTER || MODE == HJ_MODE_FULL_OUTER;     // the modes that report a row per match
    constexpr bool KEEPB = MODE == HJ_MODE_RIGHT_OUTER || MODE == HJ_MODE_FULL_OUTER || MARKING;
    static_assert(MODE != HJ_MODE_INNER && (UNIQUE || LEFTISH || KEEPB) && !(UNIQUE && KEEPB), "semi- and anti-joins walk to the first match");
    constexpr int NW = NPJ_PROBE_WAVES;
    __shared__ u64 red[4][NW];
    __shared__ u64 wave_cursor[NW];
    EmitterT<true, MATCHES ? 3 : 2> em;
    const NpjProbeColumns c = npj_probe_begin(a, em, wave_cursor);
    const uint4 *__restrict__ k4 = c.k4, *__restrict__ v4 = c.v4;
    const u64 gb = c.gb, ge = c.ge, nvec = c.nvec, stride = c.stride;
    const u64 *__restrict__ table = a.table;
    const u64 buckets = a.buckets;
    const uint32_t factor = a.factor;

    u64 acc_n = 0, acc_k = 0, acc_o = 0, acc_i = 0;
    for (u64 v = (u64)blockIdx.x * NPJ_PROBE_BLOCK + threadIdx.x; v < nvec; v += stride) {
        const uint4 kk = k4[v], vv = v4[v];
        const u64 g = v << 2;
        const uint32_t key[4] = {kk.x, kk.y, kk.z, kk.w};
        const uint32_t val[4] = {vv.x, vv.y, vv.z, vv.w};
        u64 h[4];
        bool act[4], in[4], hit[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            act[j] = (g + j >= gb) && (g + j < ge);
            in[j] = act[j]; hit[j] = false;
            h[j] = npj_bucket(key[j], factor, buckets);
        }
        if (GROUPED) {
            const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(table);
            while (act[0] | act[1] | act[2] | act[3]) {
                uint4 lo[4], hi[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {           // all group loads of the 4 chains in flight together
                    lo[j] = make_uint4(0, 0, 0, 0); hi[j] = lo[j];
                    if (act[j]) { const u64 grp = h[j] >> 2; lo[j] = t4[2 * grp]; hi[j] = t4[2 * grp + 1]; }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (act[j]) {
                        const uint32_t bk[4] = {lo[j].x, lo[j].z, hi[j].x, hi[j].z};   // keys of the group
                        const uint32_t bv[4] = {lo[j].y, lo[j].w, hi[j].y, hi[j].w};   // payloads
                        const uint32_t first = (uint32_t)h[j] & 3u;
                        bool open = true;                                              // no empty bucket seen yet
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const bool inb = open && ((uint32_t)b >= first);
                            if (inb && bk[b] == 0u) open = false;
                            else if (inb && bk[b] == key[j]) {
                                if constexpr (MATCHES) {
                                    acc_n += 1; acc_k += key[j]; acc_o += val[j]; acc_i += bv[b];
                                    em.emit(key[j], val[j], bv[b]);
                                }
                                if constexpr (KEEPB) { const u64 at = (h[j] & ~3ull) + b; atomicOr(&a.bucket_bits[at >> 5], 1u << ((uint32_t)at & 31u)); }
                                hit[j] = true;
                                if (UNIQUE) open = false;
                            }
                        }
                        if (!open) act[j] = false;
                        else { h[j] = (h[j] & ~3ull) + 4; if (h[j] >= buckets) h[j] = 0; }
                    }
                }
            }
        } else {
            u64 t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = act[j] ? table[h[j]] : 0ull;
            while (act[0] | act[1] | act[2] | act[3]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (act[j]) {
                        if ((uint32_t)t[j] == 0u) {
                            act[j] = false;
                        } else {
                            if ((uint32_t)t[j] == key[j]) {
                                const uint32_t iv = (uint32_t)(t[j] >> 32);
                                if constexpr (MATCHES) {
                                    acc_n += 1; acc_k += key[j]; acc_o += val[j]; acc_i += iv;
                                    em.emit(key[j], val[j], iv);
                                }
                                if constexpr (KEEPB) atomicOr(&a.bucket_bits[h[j] >> 5], 1u << ((uint32_t)h[j] & 31u));
                                hit[j] = true;
                                if (UNIQUE) { act[j] = false; continue; }
                            }
                            if (++h[j] == buckets) h[j] = 0;
                            t[j] = table[h[j]];
                        }
                    }
                }
            }
        }
        if constexpr (LEFTISH) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (in[j] && !hit[j]) {                 // (a probe key 0 stops at the first empty bucket: no match, a NULL row)
                    acc_n += 1; acc_k += key[j]; acc_o += val[j];
                    em.emit(key[j], val[j], HJGPU_NULL_VAL);
                }
            }
        } else if constexpr (MODE == HJ_MODE_SEMI || MODE == HJ_MODE_ANTI) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (in[j] && hit[j] == (MODE == HJ_MODE_SEMI)) {
                    acc_n += 1; acc_k += key[j]; acc_o += val[j];
                    em.emit(key[j], val[j], 0u);
                }
            }
        }
    }
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);
    hj_add_to_result(red, a.result, acc_n, acc_k, acc_o, acc_i);
}

// The inner join's walk, a body of its own ("One body per probe walk"): npj_probe_body without the modes.
template <bool GROUPED, bool UNIQUE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_probe_kernel(NpjProbeArgs a)
{
    constexpr int NW = NPJ_PROBE_BLOCK / 64;
    __shared__ u64 red[4][NW];
    __shared__ u64 wave_cursor[NW];
    Emitter em;
    const NpjProbeColumns c = npj_probe_begin(a, em, wave_cursor);
    const uint4 *__restrict__ k4 = c.k4, *__restrict__ v4 = c.v4;
    const u64 gb = c.gb, ge = c.ge, nvec = c.nvec, stride = c.stride;
    const u64 *__restrict__ table = a.table;
    const u64 buckets = a.buckets;
    const uint32_t factor = a.factor;

    u64 acc_n = 0, acc_k = 0, acc_o = 0, acc_i = 0;
    for (u64 v = (u64)blockIdx.x * NPJ_PROBE_BLOCK + threadIdx.x; v < nvec; v += stride) {
        const uint4 kk = k4[v], vv = v4[v];
        const u64 g = v << 2;
        const uint32_t key[4] = {kk.x, kk.y, kk.z, kk.w};
        const uint32_t val[4] = {vv.x, vv.y, vv.z, vv.w};
        u64 h[4];
        bool act[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            act[j] = (g + j >= gb) && (g + j < ge);
            h[j] = npj_bucket(key[j], factor, buckets);
        }
        if (GROUPED) {
            const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(table);
            while (act[0] | act[1] | act[2] | act[3]) {
                uint4 lo[4], hi[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {           // all group loads of the 4 chains in flight together
                    lo[j] = make_uint4(0, 0, 0, 0); hi[j] = lo[j];
                    if (act[j]) { const u64 grp = h[j] >> 2; lo[j] = t4[2 * grp]; hi[j] = t4[2 * grp + 1]; }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (act[j]) {
                        const uint32_t bk[4] = {lo[j].x, lo[j].z, hi[j].x, hi[j].z};   // keys of the group
                        const uint32_t bv[4] = {lo[j].y, lo[j].w, hi[j].y, hi[j].w};   // payloads
                        const uint32_t first = (uint32_t)h[j] & 3u;
                        bool open = true;                                              // no empty bucket seen yet
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const bool in = open && ((uint32_t)b >= first);
                            if (in && bk[b] == 0u) open = false;
                            else if (in && bk[b] == key[j]) {
                                acc_n += 1; acc_k += key[j]; acc_o += val[j]; acc_i += bv[b];
                                em.emit(key[j], val[j], bv[b]);
                                if (UNIQUE) open = false;
                            }
                        }
                        if (!open) act[j] = false;
                        else { h[j] = (h[j] & ~3ull) + 4; if (h[j] >= buckets) h[j] = 0; }
                    }
                }
            }
        } else {
            u64 t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = act[j] ? table[h[j]] : 0ull;
            while (act[0] | act[1] | act[2] | act[3]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (act[j]) {
                        if ((uint32_t)t[j] == 0u) {
                            act[j] = false;
                        } else {
                            if ((uint32_t)t[j] == key[j]) {
                                const uint32_t iv = (uint32_t)(t[j] >> 32);
                                acc_n += 1; acc_k += key[j]; acc_o += val[j]; acc_i += iv;
                                em.emit(key[j], val[j], iv);
                                if (UNIQUE) { act[j] = false; continue; }
                            }
                            if (++h[j] == buckets) h[j] = 0;
                            t[j] = table[h[j]];
                        }
                    }
                }
            }
        }
    }
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);
    const int wave = threadIdx.x >> 6;          // (hj_add_to_result, written out: as a call it changes this kernel's machine code)
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k);
    acc_o = wave_reduce_sum(acc_o); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_o; red[3][wave] = acc_i; }
    __syncthreads();
    if (threadIdx.x < 4) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[threadIdx.x][i];
        if (s) atomicAdd(reinterpret_cast<u64 *>(a.result) + threadIdx.x, s);
    }
}

template <bool GROUPED, int MODE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_exists_kernel(NpjProbeArgs a)
{
    npj_probe_body<GROUPED, true, MODE>(a);
}

template <bool GROUPED, bool UNIQUE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_outer_kernel(NpjProbeArgs a)
{
    npj_probe_body<GROUPED, UNIQUE, HJ_MODE_LEFT_OUTER>(a);
}

// LINE table (the library's own whole joins, hjgpu_npj*): the walk of a key starts on the
// 64-byte line of 8 buckets it hashes to, h = 8 * H(key, f, buckets / 8), instead of on an
// arbitrary bucket.  Same bucket format, same CAS build, same walk to the first empty bucket
// with every match reported (npj.cpp:204-210, 426-442) - only the hash range differs, and like
// the load factor it does not change the join result.
// The probe is COOPERATIVE: the four lanes of a quad fetch the four 16-byte quarters of one
// key's line in ONE load instruction, so the line is one L2 request and one memory-side
// request.  PMC at 64M x 1G, load 0.25 (TCC_REQ / TCC_EA0_RDREQ per probe, probe time):
//   reference hash, 32-byte groups, 2 loads per lane and chain   1.83 / 1.48   27.4 ms
//   line hash, one lane reads its whole line with 4 loads        3.59 / 1.06   29.9 ms
// a successful probe has to see the bucket AFTER its match, so with arbitrary start buckets
// every fourth probe needs a second group; and every extra load instruction is an extra L2
// request even when it hits the same line (fit: 12.9 ms per G memory-side requests + 4.5 ms
// per G L2 requests).
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t x) { return hj_dpp<CTRL>(x); }

template <int OWNER>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t x)           // the value of lane OWNER of the quad
{
    return quad_perm<OWNER * 0x55>(x);
}

// The quad's line walk of every join mode but the inner join (npj_probe_line_kernel below, for the same reason as npj_probe_kernel).
// MATERIALIZE is a template parameter on purpose: with a run-time `if (a.ok)` inside the walk loop
// the -O3 build evaluated that (uniform) test per lane at a loop header that the continuation
// re-enters with only the walking lanes enabled, and later rounds of other lanes then took the
// emit path with a.ok == NULL (memory access fault; -O1 was fine).
// MODE (HJ_MODE_*): semi- / anti-join
// (npj_exists_line_kernel) - lane 0 of the quad reports the tuple when its walk ends: on a match (`found`, SEMI) or on an empty bucket
// without one (ANTI); left outer join (npj_outer_line_kernel) - the inner join's rows, and lane 0 of the quad reports a NULL row when the
// walk ends without any match of the quad in any of its lines.
template <bool MATERIALIZE, bool UNIQUE, int MODE>
__device__ __forceinline__ void npj_probe_line_body(NpjProbeArgs a)
{
    constexpr bool LEFTISH = MODE == HJ_MODE_LEFT_OUTER || MODE == HJ_MODE_FULL_OUTER;     // as in npj_probe_body
    constexpr bool MARKING = MODE == HJ_MODE_MARK;
    constexpr bool MATCHES = LEFTISH || MODE == HJ_MODE_RIGHT_OUTER || MODE == HJ_MODE_FULL_OUTER;
    constexpr bool KEEPB = MODE == HJ_MODE_RIGHT_OUTER || MODE == HJ_MODE_FULL_OUTER || MARKING;
    static_assert(!(MARKING && MATERIALIZE), "the marking probe reports nothing");
    static_assert(MODE != HJ_MODE_INNER && (UNIQUE || LEFTISH || KEEPB) && !(UNIQUE && KEEPB), "semi- and anti-joins walk to the first match");
    constexpr int NW = NPJ_PROBE_WAVES;
    constexpr int B = 4;                                   // lines in flight per quad
    __shared__ u64 red[4][NW];
    __shared__ u64 wave_cursor[NW];
    const int wave = threadIdx.x >> 6;
    EmitterT<true, MATCHES ? 3 : 2> em;
    const NpjProbeColumns c = npj_probe_begin(a, em, wave_cursor);
    const uint4 *__restrict__ k4 = c.k4, *__restrict__ v4 = c.v4;
    const u64 gb = c.gb, ge = c.ge, nvec = c.nvec, stride = c.stride;
    const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(a.table);
    const u64 lines = a.buckets >> 3;
    const uint32_t factor = a.factor;
    const uint32_t sub = threadIdx.x & 3;                  // my quarter of the line: buckets 2*sub, 2*sub + 1

    u64 acc_n = 0, acc_k = 0, acc_o = 0, acc_i = 0;
    // left outer join: the current walk has found a match (quad-uniform).  Declared here, set only by the left outer instances: an
    // initialised local beside the walk reorders two register moves of the semi- / anti-join instances
    bool got;
    // whole waves iterate together (the quad exchanges below need all four lanes)
    for (u64 v0 = (u64)blockIdx.x * NPJ_PROBE_BLOCK + (threadIdx.x & ~63u); v0 < nvec; v0 += stride) {
        const u64 v = v0 + hj_lane();
        uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
        if (v < nvec) { kk = k4[v]; vv = v4[v]; }
        const u64 g = v << 2;
        const uint32_t kc[4] = {kk.x, kk.y, kk.z, kk.w}, vc[4] = {vv.x, vv.y, vv.z, vv.w};
        uint32_t okc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) okc[j] = (v < nvec && g + j >= gb && g + j < ge) ? 1u : 0u;

        // the quad's 16 tuples (4 lanes x 4 components), B at a time
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += B) {
            uint32_t key[B], val[B];
            bool act[B];
            u64 ln[B];
            uint4 q[B];
#pragma unroll
            for (int i = 0; i < B; ++i) {
                const int r = r0 + i, comp = r & 3;                     // static after unrolling
                // the tuple's owner is lane r / 4 of the quad: broadcast its key, payload and validity
                if (r < 4) { key[i] = quad_perm<0x00>(kc[comp]); val[i] = quad_perm<0x00>(vc[comp]); act[i] = quad_perm<0x00>(okc[comp]) != 0; }
                else if (r < 8) { key[i] = quad_perm<0x55>(kc[comp]); val[i] = quad_perm<0x55>(vc[comp]); act[i] = quad_perm<0x55>(okc[comp]) != 0; }
                else if (r < 12) { key[i] = quad_perm<0xAA>(kc[comp]); val[i] = quad_perm<0xAA>(vc[comp]); act[i] = quad_perm<0xAA>(okc[comp]) != 0; }
                else { key[i] = quad_perm<0xFF>(kc[comp]); val[i] = quad_perm<0xFF>(vc[comp]); act[i] = quad_perm<0xFF>(okc[comp]) != 0; }
                ln[i] = npj_bucket(key[i], factor, lines);
                q[i] = make_uint4(0, 0, 0, 0);
                if (act[i]) {
                    q[i] = t4[4 * ln[i] + sub];                         // 4 lanes x 16 bytes = the key's line
                }
            }
#pragma unroll
            for (int i = 0; i < B; ++i) {
                if constexpr (LEFTISH) got = false;
                while (act[i]) {                                        // uniform inside the quad
                    // first empty bucket of the line, over the quad
                    uint32_t fe = q[i].x == 0u ? 2 * sub : (q[i].z == 0u ? 2 * sub + 1 : 8u);
                    fe = min(fe, quad_perm<0xB1>(fe));                  // lanes 0<->1, 2<->3
                    fe = min(fe, quad_perm<0x4E>(fe));                  // lanes 0<->2, 1<->3
                    bool m0 = q[i].x == key[i] && 2 * sub < fe;
                    bool m1 = q[i].z == key[i] && 2 * sub + 1 < fe;
                    bool found = false;                                 // UNIQUE: some lane of the quad holds a match
                    if (UNIQUE) {
                        // only the FIRST match of the walk counts: the lowest matching bucket of the line
                        uint32_t fm = m0 ? 2 * sub : (m1 ? 2 * sub + 1 : 8u);
                        const uint32_t mine = fm;
                        fm = min(fm, quad_perm<0xB1>(fm));
                        fm = min(fm, quad_perm<0x4E>(fm));
                        found = fm < 8u;
                        m0 = m0 && mine == fm && fm == 2 * sub;
                        m1 = m1 && mine == fm && fm == 2 * sub + 1;
                    }
                    if constexpr (MATCHES) {
                        const uint32_t m = (m0 ? 1u : 0u) + (m1 ? 1u : 0u);
                        acc_n += m; acc_k += (u64)key[i] * m; acc_o += (u64)val[i] * m;
                        acc_i += (m0 ? q[i].y : 0u); acc_i += (m1 ? q[i].w : 0u);
                        if (MATERIALIZE) {
                            if (m0) em.emit(key[i], val[i], q[i].y);
                            if (m1) em.emit(key[i], val[i], q[i].w);
                        }
                        if constexpr (KEEPB) {
                            // my two buckets of the line: 8 * line + 2 * sub and the next one - an even index, both bits in one word
                            const u64 at = 8 * ln[i] + 2 * sub;
                            if (m0 || m1) atomicOr(&a.bucket_bits[at >> 5], ((m0 ? 1u : 0u) | (m1 ? 2u : 0u)) << ((uint32_t)at & 31u));
                        }
                    } else if constexpr (MARKING) {
                        const u64 at = 8 * ln[i] + 2 * sub;                     // as above
                        if (m0 || m1) atomicOr(&a.bucket_bits[at >> 5], ((m0 ? 1u : 0u) | (m1 ? 2u : 0u)) << ((uint32_t)at & 31u));
                    } else if (fe < 8u || found) {
                        if (sub == 0 && found == (MODE == HJ_MODE_SEMI)) {
                            acc_n += 1; acc_k += key[i]; acc_o += val[i];
                            if (MATERIALIZE) em.emit(key[i], val[i], 0u);
                        }
                    }
                    if constexpr (LEFTISH) {
                        if (UNIQUE) got = got || found;
                        else {
                            uint32_t any = (m0 || m1) ? 1u : 0u;                // a match anywhere in the quad's line
                            any |= quad_perm<0xB1>(any);
                            any |= quad_perm<0x4E>(any);
                            got = got || any != 0u;
                        }
                        if ((fe < 8u || (UNIQUE && found)) && !got && sub == 0) {
                            acc_n += 1; acc_k += key[i]; acc_o += val[i];
                            if (MATERIALIZE) em.emit(key[i], val[i], HJGPU_NULL_VAL);
                        }
                    }
                    if (fe < 8u || (UNIQUE && found)) break;            // the walk ends at the first empty bucket (UNIQUE: first match)
                    if (++ln[i] == lines) ln[i] = 0;                    // full line: the walk goes on in the next one
                    q[i] = t4[4 * ln[i] + sub];
                }
            }
        }
    }
    if (MATERIALIZE) hj_leave_cursor(a.final_offsets, wave_cursor);
    // (hj_add_to_result, written out: as a call it reorders two register moves at the head of the semi- / anti-join instances' loop)
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k);
    acc_o = wave_reduce_sum(acc_o); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_o; red[3][wave] = acc_i; }
    __syncthreads();
    if (threadIdx.x < 4) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[threadIdx.x][i];
        if (s) atomicAdd(reinterpret_cast<u64 *>(a.result) + threadIdx.x, s);
    }
}

// The inner join's line walk, a body of its own ("One body per probe walk"): npj_probe_line_body without the modes.
template <bool MATERIALIZE, bool UNIQUE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_probe_line_kernel(NpjProbeArgs a)
{
    constexpr int NW = NPJ_PROBE_BLOCK / 64;
    constexpr int B = 4;                                   // lines in flight per quad
    __shared__ u64 red[4][NW];
    __shared__ u64 wave_cursor[NW];
    const int wave = threadIdx.x >> 6;
    Emitter em;
    const NpjProbeColumns c = npj_probe_begin(a, em, wave_cursor);
    const uint4 *__restrict__ k4 = c.k4, *__restrict__ v4 = c.v4;
    const u64 gb = c.gb, ge = c.ge, nvec = c.nvec, stride = c.stride;
    const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(a.table);
    const u64 lines = a.buckets >> 3;
    const uint32_t factor = a.factor;
    const uint32_t sub = threadIdx.x & 3;                  // my quarter of the line: buckets 2*sub, 2*sub + 1

    u64 acc_n = 0, acc_k = 0, acc_o = 0, acc_i = 0;
    // whole waves iterate together (the quad exchanges below need all four lanes)
    for (u64 v0 = (u64)blockIdx.x * NPJ_PROBE_BLOCK + (threadIdx.x & ~63u); v0 < nvec; v0 += stride) {
        const u64 v = v0 + hj_lane();
        uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
        if (v < nvec) { kk = k4[v]; vv = v4[v]; }
        const u64 g = v << 2;
        const uint32_t kc[4] = {kk.x, kk.y, kk.z, kk.w}, vc[4] = {vv.x, vv.y, vv.z, vv.w};
        uint32_t okc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) okc[j] = (v < nvec && g + j >= gb && g + j < ge) ? 1u : 0u;

        // the quad's 16 tuples (4 lanes x 4 components), B at a time
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += B) {
            uint32_t key[B], val[B];
            bool act[B];
            u64 ln[B];
            uint4 q[B];
#pragma unroll
            for (int i = 0; i < B; ++i) {
                const int r = r0 + i, comp = r & 3;                     // static after unrolling
                // the tuple's owner is lane r / 4 of the quad: broadcast its key, payload and validity
                if (r < 4) { key[i] = quad_perm<0x00>(kc[comp]); val[i] = quad_perm<0x00>(vc[comp]); act[i] = quad_perm<0x00>(okc[comp]) != 0; }
                else if (r < 8) { key[i] = quad_perm<0x55>(kc[comp]); val[i] = quad_perm<0x55>(vc[comp]); act[i] = quad_perm<0x55>(okc[comp]) != 0; }
                else if (r < 12) { key[i] = quad_perm<0xAA>(kc[comp]); val[i] = quad_perm<0xAA>(vc[comp]); act[i] = quad_perm<0xAA>(okc[comp]) != 0; }
                else { key[i] = quad_perm<0xFF>(kc[comp]); val[i] = quad_perm<0xFF>(vc[comp]); act[i] = quad_perm<0xFF>(okc[comp]) != 0; }
                ln[i] = npj_bucket(key[i], factor, lines);
                q[i] = make_uint4(0, 0, 0, 0);
                if (act[i]) {
                    q[i] = t4[4 * ln[i] + sub];                         // 4 lanes x 16 bytes = the key's line
                }
            }
#pragma unroll
            for (int i = 0; i < B; ++i) {
                while (act[i]) {                                        // uniform inside the quad
                    // first empty bucket of the line, over the quad
                    uint32_t fe = q[i].x == 0u ? 2 * sub : (q[i].z == 0u ? 2 * sub + 1 : 8u);
                    fe = min(fe, quad_perm<0xB1>(fe));                  // lanes 0<->1, 2<->3
                    fe = min(fe, quad_perm<0x4E>(fe));                  // lanes 0<->2, 1<->3
                    bool m0 = q[i].x == key[i] && 2 * sub < fe;
                    bool m1 = q[i].z == key[i] && 2 * sub + 1 < fe;
                    bool found = false;                                 // UNIQUE: some lane of the quad holds a match
                    if (UNIQUE) {
                        // only the FIRST match of the walk counts: the lowest matching bucket of the line
                        uint32_t fm = m0 ? 2 * sub : (m1 ? 2 * sub + 1 : 8u);
                        const uint32_t mine = fm;
                        fm = min(fm, quad_perm<0xB1>(fm));
                        fm = min(fm, quad_perm<0x4E>(fm));
                        found = fm < 8u;
                        m0 = m0 && mine == fm && fm == 2 * sub;
                        m1 = m1 && mine == fm && fm == 2 * sub + 1;
                    }
                    const uint32_t m = (m0 ? 1u : 0u) + (m1 ? 1u : 0u);
                    acc_n += m; acc_k += (u64)key[i] * m; acc_o += (u64)val[i] * m;
                    acc_i += (m0 ? q[i].y : 0u); acc_i += (m1 ? q[i].w : 0u);
                    if (MATERIALIZE) {
                        if (m0) em.emit(key[i], val[i], q[i].y);
                        if (m1) em.emit(key[i], val[i], q[i].w);
                    }
                    if (fe < 8u || (UNIQUE && found)) break;            // the walk ends at the first empty bucket (UNIQUE: first match)
                    if (++ln[i] == lines) ln[i] = 0;                    // full line: the walk goes on in the next one
                    q[i] = t4[4 * ln[i] + sub];
                }
            }
        }
    }
    if (MATERIALIZE) hj_leave_cursor(a.final_offsets, wave_cursor);
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k);
    acc_o = wave_reduce_sum(acc_o); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_o; red[3][wave] = acc_i; }
    __syncthreads();
    if (threadIdx.x < 4) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[threadIdx.x][i];
        if (s) atomicAdd(reinterpret_cast<u64 *>(a.result) + threadIdx.x, s);
    }
}

template <bool MATERIALIZE, int MODE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_exists_line_kernel(NpjProbeArgs a)
{
    npj_probe_line_body<MATERIALIZE, true, MODE>(a);
}

template <bool MATERIALIZE, bool UNIQUE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_outer_line_kernel(NpjProbeArgs a)
{
    npj_probe_line_body<MATERIALIZE, UNIQUE, HJ_MODE_LEFT_OUTER>(a);
}

// Right and full outer joins (HJGPU_FLAG_RIGHT_OUTER / _FULL_OUTER): the inner / left outer probes, marking every bucket they match
// (NpjProbeArgs::bucket_bits).  Kernels of their own names; never UNIQUE.
template <bool GROUPED>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_right_kernel(NpjProbeArgs a)
{
    npj_probe_body<GROUPED, false, HJ_MODE_RIGHT_OUTER>(a);
}

template <bool GROUPED>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_full_kernel(NpjProbeArgs a)
{
    npj_probe_body<GROUPED, false, HJ_MODE_FULL_OUTER>(a);
}

template <bool MATERIALIZE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_right_line_kernel(NpjProbeArgs a)
{
    npj_probe_line_body<MATERIALIZE, false, HJ_MODE_RIGHT_OUTER>(a);
}

template <bool MATERIALIZE>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_full_line_kernel(NpjProbeArgs a)
{
    npj_probe_line_body<MATERIALIZE, false, HJ_MODE_FULL_OUTER>(a);
}

// The probes of right semi- and anti-joins (HJGPU_FLAG_RIGHT_SEMI / _RIGHT_ANTI): the full walk - one bucket per build tuple, every copy
// of a key is visited -, marking every bucket it matches and reporting nothing (HJ_MODE_MARK).  Launched without output columns.
template <bool GROUPED>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_mark_kernel(NpjProbeArgs a)
{
    npj_probe_body<GROUPED, false, HJ_MODE_MARK>(a);
}

__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_mark_line_kernel(NpjProbeArgs a)
{
    npj_probe_line_body<false, false, HJ_MODE_MARK>(a);
}

// The tail of a right / full outer NPJ join, behind the probe with the probe's grid: scans the table (four buckets = 2 x 16 bytes and
// their four bits per lane and step; buckets is a multiple of 8) and reports every tuple (key != 0) whose bucket's bit is clear as
// (key, HJGPU_NULL_VAL, inner_val).  `resume`: the waves go on in the output blocks the probe's waves left open.
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_unmatched_kernel(NpjProbeArgs a, uint32_t resume)
{
    constexpr int NW = NPJ_PROBE_WAVES;
    __shared__ u64 red[3][NW];
    __shared__ u64 wave_cursor[NW];
    const int wave = threadIdx.x >> 6;
    Emitter em;
    em.init(a.ok, a.oov, a.oiv, a.block_size, a.block_limit, a.block_counter, a.overflow, &wave_cursor[wave]);
    if (hj_lane() == 0) wave_cursor[wave] = (a.ok && resume) ? a.final_offsets[(u64)blockIdx.x * NW + wave] : HJ_NO_CURSOR;
    const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(a.table);
    const uint32_t *__restrict__ bits = a.bucket_bits;
    const u64 nvec = a.buckets >> 2, stride = (u64)gridDim.x * NPJ_PROBE_BLOCK;
    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    for (u64 v = (u64)blockIdx.x * NPJ_PROBE_BLOCK + threadIdx.x; v < nvec; v += stride) {
        const uint4 x = t4[2 * v], y = t4[2 * v + 1];
        const uint32_t seen = bits[v >> 3] >> (((uint32_t)v & 7u) * 4);      // buckets 4v ... 4v + 3
        const uint32_t key[4] = {x.x, x.z, y.x, y.z}, val[4] = {x.y, x.w, y.y, y.w};
        uint32_t rep = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool r = key[j] != 0u && !((seen >> j) & 1u);
            rep |= r ? 1u << j : 0u;
            acc_n += r ? 1u : 0u; acc_k += r ? key[j] : 0u; acc_i += r ? val[j] : 0u;
        }
        if (a.ok) {
            const uint32_t none[4] = {HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL};
            if (rep == 15u && a.block_size >= 512) em.emit4(key, none, val);       // (emit4: blocks of 512 rows and more)
            else if (rep) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((rep >> j) & 1u) em.emit(key[j], HJGPU_NULL_VAL, val[j]);
            }
        }
    }
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);
    // (three sums, written out: the reduction as a call changes the schedule of this kernel, see hj_add_to_result)
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_i; }
    __syncthreads();
    if (threadIdx.x < 3) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[threadIdx.x][i];
        if (s) atomicAdd(reinterpret_cast<u64 *>(a.result) + (threadIdx.x == 2 ? 3 : threadIdx.x), s);     // count, sum_keys, sum_inner_vals
    }
}

int hj_launch_npj_unmatched(const NpjProbeArgs &a, int grid, bool resume, hipStream_t stream)
{
    if (!a.bucket_bits || a.buckets % 8 != 0 || ((uintptr_t)a.table & 15) || grid < 1 || (a.ok && !a.final_offsets)) return HJGPU_EINVAL;
    hipLaunchKernelGGL(npj_unmatched_kernel, dim3(grid), dim3(NPJ_PROBE_BLOCK), 0, stream, a, resume ? 1u : 0u);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// The tail of a right semi- / anti-join, npj_unmatched_kernel's sibling: the same scan of the table.  `flip` = 0: the tuples whose bucket's
// bit is clear (right anti-join); ~0: those whose bit is set (right semi-join).  Rows of two columns, (key, inner_val): a.oiv is the
// emitter's second column, a.oov is not touched.  The probe has reported nothing: every wave starts without an open block.
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_rows_kernel(NpjProbeArgs a, uint32_t flip)
{
    constexpr int NW = NPJ_PROBE_WAVES;
    __shared__ u64 red[3][NW];
    __shared__ u64 wave_cursor[NW];
    const int wave = threadIdx.x >> 6;
    EmitterT<true, 2> em;
    em.init(a.ok, a.oiv, nullptr, a.block_size, a.block_limit, a.block_counter, a.overflow, &wave_cursor[wave]);
    if (hj_lane() == 0) wave_cursor[wave] = HJ_NO_CURSOR;
    const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(a.table);
    const uint32_t *__restrict__ bits = a.bucket_bits;
    const u64 nvec = a.buckets >> 2, stride = (u64)gridDim.x * NPJ_PROBE_BLOCK;
    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    for (u64 v = (u64)blockIdx.x * NPJ_PROBE_BLOCK + threadIdx.x; v < nvec; v += stride) {
        const uint4 x = t4[2 * v], y = t4[2 * v + 1];
        const uint32_t skip = (bits[v >> 3] ^ flip) >> (((uint32_t)v & 7u) * 4);      // buckets 4v ... 4v + 3
        const uint32_t key[4] = {x.x, x.z, y.x, y.z}, val[4] = {x.y, x.w, y.y, y.w};
        uint32_t rep = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool r = key[j] != 0u && !((skip >> j) & 1u);
            rep |= r ? 1u << j : 0u;
            acc_n += r ? 1u : 0u; acc_k += r ? key[j] : 0u; acc_i += r ? val[j] : 0u;
        }
        if (a.ok) {
            if (rep == 15u && a.block_size >= 512) em.emit4(key, val, val);        // (emit4: blocks of 512 rows and more)
            else if (rep) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((rep >> j) & 1u) em.emit(key[j], val[j], 0u);
            }
        }
    }
    if (a.ok) hj_leave_cursor(a.final_offsets, wave_cursor);
    acc_n = wave_reduce_sum(acc_n); acc_k = wave_reduce_sum(acc_k); acc_i = wave_reduce_sum(acc_i);
    if (hj_lane() == 0) { red[0][wave] = acc_n; red[1][wave] = acc_k; red[2][wave] = acc_i; }
    __syncthreads();
    if (threadIdx.x < 3) {
        u64 s = 0;
        for (int i = 0; i < NW; ++i) s += red[threadIdx.x][i];
        if (s) atomicAdd(reinterpret_cast<u64 *>(a.result) + (threadIdx.x == 2 ? 3 : threadIdx.x), s);     // count, sum_keys, sum_inner_vals
    }
}

int hj_launch_npj_rows(const NpjProbeArgs &a, int grid, hipStream_t stream)
{
    if (!hj_mode_reports_build(a.mode) || !a.bucket_bits || a.buckets % 8 != 0 || ((uintptr_t)a.table & 15) || grid < 1 ||
        (a.ok && (!a.final_offsets || !a.oiv))) return HJGPU_EINVAL;
    hipLaunchKernelGGL(npj_rows_kernel, dim3(grid), dim3(NPJ_PROBE_BLOCK), 0, stream, a, a.mode == HJ_MODE_RIGHT_SEMI ? ~0u : 0u);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_npj_probe_grid(int cus, size_t n)
{
    u64 blocks = ((n + 3) / 4 + NPJ_PROBE_BLOCK - 1) / NPJ_PROBE_BLOCK;
    if (blocks > (u64)cus * 8) blocks = (u64)cus * 8;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// The probe kernel of a join mode.  LINE: the line walk, else the bucket / group walk; X: the walk's first template argument
// (MATERIALIZE / GROUPED); U: the first-match walk (semi- and anti-joins always, right and full outer joins never).
typedef void (*NpjProbeKernel)(NpjProbeArgs);
template <bool LINE, bool X, bool U>
static NpjProbeKernel npj_probe_kernel_of(uint32_t mode)
{
    switch (mode) {
    case HJ_MODE_SEMI: return LINE ? npj_exists_line_kernel<X, HJ_MODE_SEMI> : npj_exists_kernel<X, HJ_MODE_SEMI>;
    case HJ_MODE_ANTI: return LINE ? npj_exists_line_kernel<X, HJ_MODE_ANTI> : npj_exists_kernel<X, HJ_MODE_ANTI>;
    case HJ_MODE_LEFT_OUTER: return LINE ? npj_outer_line_kernel<X, U> : npj_outer_kernel<X, U>;
    case HJ_MODE_RIGHT_OUTER: return LINE ? npj_right_line_kernel<X> : npj_right_kernel<X>;
    case HJ_MODE_FULL_OUTER: return LINE ? npj_full_line_kernel<X> : npj_full_kernel<X>;
    case HJ_MODE_RIGHT_SEMI:
    case HJ_MODE_RIGHT_ANTI: return LINE ? npj_mark_line_kernel : npj_mark_kernel<X>;      // (launched without output columns)
    default: return LINE ? npj_probe_line_kernel<X, U> : npj_probe_kernel<X, U>;
    }
}

int hj_launch_npj_probe(const NpjProbeArgs &a, int cus, hipStream_t stream, int *grid_out)
{
    const int grid = hj_npj_probe_grid(cus, a.n);
    if (grid_out) *grid_out = grid;
    if (hj_mode_keeps_build(a.mode) && (a.unique || !a.bucket_bits)) return HJGPU_EINVAL;
    // right semi- / anti-joins: the marking probe - launched without output columns (the tail has the rows), never the first-match walk
    NpjProbeArgs b = a;
    if (hj_mode_reports_build(a.mode)) {
        if (!a.bucket_bits) return HJGPU_EINVAL;
        b.ok = nullptr; b.unique = 0;
    }
    if (b.line_hash && (b.buckets % 8 != 0 || ((uintptr_t)b.table & 63))) return HJGPU_EINVAL;
    const bool grouped = (b.buckets % 4 == 0) && (((uintptr_t)b.table & 31) == 0);
    NpjProbeKernel kernel = nullptr;
    hj_with_bool(b.line_hash != 0, [&](auto line) {
        hj_with_bool(line ? b.ok != nullptr : grouped, [&](auto x) {
            hj_with_bool(b.unique != 0, [&](auto u) { kernel = npj_probe_kernel_of<decltype(line)::value, decltype(x)::value, decltype(u)::value>(b.mode); });
        });
    });
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NPJ_PROBE_BLOCK), 0, stream, b);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// --------------------------------------------------------------------------
// Positional look-up (hjgpu_npj_lookup*, DESIGN.md section 5 "Positional look-up"): out[i] = the payload of the first build tuple the walk
// of probe key i meets (HJGPU_NULL_VAL: none), bit i of the bitmap = it met one - both IN THE PROBE COLUMN'S ORDER.  No probe payloads,
// no emitter, no block claims: lane L of a wave trip owns rows 4 L ... 4 L + 3 of the trip's 256 consecutive rows, ends the trip with
// their four answers and a nibble of match bits, and writes one 16-byte vector; the nibbles of 8 lanes make one word of the bitmap.
// Bodies of their own beside the join walks (which stay as they are, instruction for instruction); the epilogue is the shared
// hj_add_to_result.  The key column is 16-byte aligned (the entry points refuse anything else): vector v holds rows 4 v ... 4 v + 3.
// VALS / BITS are template parameters for npj_probe_line_body's reason for MATERIALIZE, and so that no store sits behind a run-time flag
// (tests/test_store_policy_isa.py); <false, false> is the aggregate-only instance.
// Selected look-up (hjgpu_lookup_selected*, hjgpu_npj_lookup_table_selected; DESIGN.md section 5 "Selected look-up"), SEL: the same walks
// for the rows whose bit is set in select_bits.  An unselected row is never active: no load of the table is issued for it, it leaves as
// HJGPU_NULL_VAL with bit 0 and is counted nowhere.  One body per walk behind thin named kernels (DESIGN.md "One body per look-up walk");
// the head and the end of a trip are hj_lookup.hpp's, where the in-place rule (match_bits == select_bits) is kept.  The head hands every
// lane the nibble of its rows that are to be looked up: the select bits with SEL, the rows below n without.
// NPJ_SEL_BATCH wave trips per loop iteration of a selected kernel: their select words are loaded first, then their keys; a plain kernel
// makes one trip per iteration.
// --------------------------------------------------------------------------
constexpr int NPJ_SEL_BATCH = 2;

// The line walk for ONE owner lane of the quad: its four keys, all four lines in flight - the quad walk of npj_probe_line_body with the
// first-match rule, without the payload column.  `look` is the owner's nibble of rows to look up.  After its walk a key has its answer in
// ONE lane - the one whose bucket is the first match - and a quad OR of (mine ? payload : 0) takes it to the owner (`got` is quad-uniform
// already: it comes out of the quad's min-reduction of the first matching bucket).  A quad none of whose owner's keys is to be looked up
// skips the round; where that holds for every quad of the wave the round issues nothing.
template <int OWNER>
__device__ __forceinline__ void npj_line_round(const uint4 *__restrict__ t4, u64 lines, uint32_t factor, uint32_t sub, const uint32_t (&kc)[4],
                                               uint32_t look, uint32_t (&res)[4], uint32_t &nib)
{
    const uint32_t on = quad_bcast<OWNER>(look);                    // the owner's nibble: quad-uniform
    if (on == 0u) return;
    uint32_t key[4];
    bool act[4];
    u64 ln[4];
    uint4 q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        key[i] = quad_bcast<OWNER>(kc[i]);
        act[i] = (on >> i) & 1u;
        ln[i] = npj_bucket(key[i], factor, lines);
        q[i] = make_uint4(0, 0, 0, 0);
        if (act[i]) q[i] = t4[4 * ln[i] + sub];                     // 4 lanes x 16 bytes = the key's line
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t pay = 0;                                           // the first match's payload, in the lane that holds its bucket
        bool got = false;                                           // the walk found a match (quad-uniform)
        while (act[i]) {                                            // uniform inside the quad
            uint32_t fe = q[i].x == 0u ? 2 * sub : (q[i].z == 0u ? 2 * sub + 1 : 8u);      // first empty bucket of the line, over the quad
            fe = min(fe, quad_perm<0xB1>(fe));                      // lanes 0<->1, 2<->3
            fe = min(fe, quad_perm<0x4E>(fe));                      // lanes 0<->2, 1<->3
            const bool m0 = q[i].x == key[i] && 2 * sub < fe;
            const bool m1 = q[i].z == key[i] && 2 * sub + 1 < fe;
            uint32_t fm = m0 ? 2 * sub : (m1 ? 2 * sub + 1 : 8u);   // only the FIRST match counts: the lowest matching bucket of the line
            const uint32_t mine = fm;
            fm = min(fm, quad_perm<0xB1>(fm));
            fm = min(fm, quad_perm<0x4E>(fm));
            got = fm < 8u;
            if (got && mine == fm) pay = m0 ? q[i].y : q[i].w;
            if (fe < 8u || got) break;                              // the walk ends at the first match or the first empty bucket
            if (++ln[i] == lines) ln[i] = 0;                        // full line: the walk goes on in the next one
            q[i] = t4[4 * ln[i] + sub];
        }
        pay |= quad_perm<0xB1>(pay);                                // to the owner (a probe key 0: no match, pay 0)
        pay |= quad_perm<0x4E>(pay);
        if (got && sub == (uint32_t)OWNER) { res[i] = pay; nib |= 1u << i; }
    }
}

// The library's own line-hashed tables: the quad's 16 keys (4 lanes x 4 components) in four rounds, one per owner lane
template <bool SEL, bool VALS, bool BITS>
__device__ __forceinline__ void npj_lookup_line_body(const NpjLookupArgs &a, const uint32_t *select_bits)
{
    constexpr int NW = NPJ_PROBE_WAVES;
    constexpr int BATCH = SEL ? NPJ_SEL_BATCH : 1;
    __shared__ u64 red[4][NW];
    const uint4 *__restrict__ k4 = reinterpret_cast<const uint4 *>(a.keys);
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * NPJ_PROBE_BLOCK;
    const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(a.table);
    const u64 lines = a.buckets >> 3;
    const uint32_t factor = a.factor;
    const uint32_t sub = threadIdx.x & 3;                  // my quarter of the line: buckets 2*sub, 2*sub + 1

    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    // whole waves iterate together (the quad exchanges and the bitmaps' words need all lanes)
    for (u64 v0 = (u64)blockIdx.x * NPJ_PROBE_BLOCK + (threadIdx.x & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t look[BATCH];
        uint4 kk[BATCH];
        lookup_fetch<SEL, BATCH, SEL>(select_bits, k4, v0, stride, n, look, kk);
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            if (v0 + (u64)u * stride >= nvec) break;                     // the wave's trip lies beyond the column (the same for all its lanes)
            const u64 v = v0 + (u64)u * stride + hj_lane();
            const uint32_t kc[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
            uint32_t res[4] = {HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL};
            uint32_t nib = 0;
            bool any = true;
            if constexpr (SEL) any = __ballot(look[u] != 0u) != 0ull;    // a trip without a selected row: straight to the stores
            if (any) {
                npj_line_round<0>(t4, lines, factor, sub, kc, look[u], res, nib);
                npj_line_round<1>(t4, lines, factor, sub, kc, look[u], res, nib);
                npj_line_round<2>(t4, lines, factor, sub, kc, look[u], res, nib);
                npj_line_round<3>(t4, lines, factor, sub, kc, look[u], res, nib);
            }
            lookup_leave<VALS, BITS>(a.vals_out, a.match_bits, n, v, kc, res, nib, acc_n, acc_k, acc_i);
        }
    }
    hj_add_to_result(red, a.result, acc_n, acc_k, 0ull, acc_i);
}

template <bool VALS, bool BITS>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_lookup_line_kernel(NpjLookupArgs a)
{
    npj_lookup_line_body<false, VALS, BITS>(a, nullptr);
}

template <bool VALS, bool BITS>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_lookup_sel_line_kernel(NpjLookupSelArgs a)
{
    npj_lookup_line_body<true, VALS, BITS>(a, a.select_bits);
}

// Tables with the reference's hash (hjgpu_npj_lookup_table*; whole look-ups under option "npj_refhash"): the bucket / group walk of
// npj_probe_body with the first-match rule.  Every lane walks its own four rows: nothing to route.  GROUPED as there.  The two walks stand
// in the body itself: behind a function of their own the grouped one compiled to a quarter more instructions and a wave per SIMD less.
template <bool SEL, bool GROUPED, bool VALS, bool BITS>
__device__ __forceinline__ void npj_lookup_body(const NpjLookupArgs &a, const uint32_t *select_bits)
{
    constexpr int NW = NPJ_PROBE_WAVES;
    constexpr int BATCH = SEL ? NPJ_SEL_BATCH : 1;
    __shared__ u64 red[4][NW];
    const uint4 *__restrict__ k4 = reinterpret_cast<const uint4 *>(a.keys);
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * NPJ_PROBE_BLOCK;
    const u64 *__restrict__ table = a.table;
    const u64 buckets = a.buckets;
    const uint32_t factor = a.factor;

    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    // whole waves iterate together (the bitmaps' words need all lanes)
    for (u64 v0 = (u64)blockIdx.x * NPJ_PROBE_BLOCK + (threadIdx.x & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t look[BATCH];
        uint4 kk[BATCH];
        lookup_fetch<SEL, BATCH, SEL>(select_bits, k4, v0, stride, n, look, kk);
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            if (v0 + (u64)u * stride >= nvec) break;                     // the wave's trip lies beyond the column (the same for all its lanes)
            const u64 v = v0 + (u64)u * stride + hj_lane();
            const uint32_t key[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
            uint32_t res[4] = {HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL, HJGPU_NULL_VAL};
            uint32_t nib = 0;
            u64 h[4];
            bool act[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                act[j] = (look[u] >> j) & 1u;
                h[j] = npj_bucket(key[j], factor, buckets);
            }
            if (GROUPED) {
                const uint4 *__restrict__ t4 = reinterpret_cast<const uint4 *>(table);
                while (act[0] | act[1] | act[2] | act[3]) {
                    uint4 lo[4], hi[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {           // all group loads of the 4 chains in flight together
                        lo[j] = make_uint4(0, 0, 0, 0); hi[j] = lo[j];
                        if (act[j]) { const u64 grp = h[j] >> 2; lo[j] = t4[2 * grp]; hi[j] = t4[2 * grp + 1]; }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (act[j]) {
                            const uint32_t bk[4] = {lo[j].x, lo[j].z, hi[j].x, hi[j].z};   // keys of the group
                            const uint32_t bv[4] = {lo[j].y, lo[j].w, hi[j].y, hi[j].w};   // payloads
                            const uint32_t first = (uint32_t)h[j] & 3u;
                            bool open = true;                                              // neither an empty bucket nor a match seen yet
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const bool inb = open && ((uint32_t)b >= first);
                                if (inb && bk[b] == 0u) open = false;
                                else if (inb && bk[b] == key[j]) { res[j] = bv[b]; nib |= 1u << j; open = false; }
                            }
                            if (!open) act[j] = false;
                            else { h[j] = (h[j] & ~3ull) + 4; if (h[j] >= buckets) h[j] = 0; }
                        }
                    }
                }
            } else {
                u64 t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = act[j] ? table[h[j]] : 0ull;
                while (act[0] | act[1] | act[2] | act[3]) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (act[j]) {
                            if ((uint32_t)t[j] == 0u) {
                                act[j] = false;
                            } else if ((uint32_t)t[j] == key[j]) {
                                res[j] = (uint32_t)(t[j] >> 32); nib |= 1u << j;
                                act[j] = false;
                            } else {
                                if (++h[j] == buckets) h[j] = 0;
                                t[j] = table[h[j]];
                            }
                        }
                    }
                }
            }
            lookup_leave<VALS, BITS>(a.vals_out, a.match_bits, n, v, key, res, nib, acc_n, acc_k, acc_i);
        }
    }
    hj_add_to_result(red, a.result, acc_n, acc_k, 0ull, acc_i);
}

template <bool GROUPED, bool VALS, bool BITS>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_lookup_kernel(NpjLookupArgs a)
{
    npj_lookup_body<false, GROUPED, VALS, BITS>(a, nullptr);
}

template <bool GROUPED, bool VALS, bool BITS>
__global__ __launch_bounds__(NPJ_PROBE_BLOCK) void npj_lookup_sel_kernel(NpjLookupSelArgs a)
{
    npj_lookup_body<true, GROUPED, VALS, BITS>(a, a.select_bits);
}

// a.select_bits == NULL: the plain kernels on the base slice of the arguments
int hj_launch_npj_lookup(const NpjLookupSelArgs &a, int cus, hipStream_t stream)
{
    if (a.n == 0) return HJGPU_OK;
    if (!a.keys || !a.table || !a.result || a.buckets == 0) return HJGPU_EINVAL;
    if ((((uintptr_t)a.keys | (uintptr_t)a.vals_out | (uintptr_t)a.match_bits | (uintptr_t)a.select_bits) & 15) || ((uintptr_t)a.table & 7)) return HJGPU_EINVAL;
    if (a.line_hash && (a.buckets % 8 != 0 || ((uintptr_t)a.table & 63))) return HJGPU_EINVAL;
    const int grid = hj_npj_probe_grid(cus, a.n);
    const bool grouped = (a.buckets % 4 == 0) && (((uintptr_t)a.table & 31) == 0);
    void (*plain)(NpjLookupArgs) = nullptr;
    void (*selected)(NpjLookupSelArgs) = nullptr;
    hj_with_bool(a.vals_out != nullptr, [&](auto vals) {
        hj_with_bool(a.match_bits != nullptr, [&](auto bits) {
            constexpr bool V = decltype(vals)::value, M = decltype(bits)::value;
            plain = a.line_hash ? npj_lookup_line_kernel<V, M> : grouped ? npj_lookup_kernel<true, V, M> : npj_lookup_kernel<false, V, M>;
            selected = a.line_hash ? npj_lookup_sel_line_kernel<V, M> : grouped ? npj_lookup_sel_kernel<true, V, M> : npj_lookup_sel_kernel<false, V, M>;
        });
    });
    if (a.select_bits) hipLaunchKernelGGL(selected, dim3(grid), dim3(NPJ_PROBE_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(plain, dim3(grid), dim3(NPJ_PROBE_BLOCK), 0, stream, static_cast<const NpjLookupArgs &>(a));
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// --------------------------------------------------------------------------
// K9 close_gaps (npj.cpp:475-514).  Input: one end cursor per worker (wave);
// [cursor, end of its block) is a hole.  The filled region is made the dense
// prefix [0, J): tuples are taken from the highest filled positions and moved
// into the lowest holes.  Plan kernel (one workgroup): sort the holes (bitonic,
// LDS), then the reference's two-pointer walk (thread 0; <= 2*#workers steps)
// emits a move list; copy kernel: the whole chip executes the moves.  J is
// written to *dense_count.
// --------------------------------------------------------------------------
constexpr int CG_BLOCK = 1024;
constexpr int CG_MAX = 8192;      // max workers (waves) supported

struct Move { u64 dst, src, cnt; };

// Plan, in parallel.  Sort the holes by position (bitonic, LDS).  With top = end of the highest
// hole's block (the highest claimed block is some worker's last block: nothing filled lies above
// it), J = top - sum of the holes is the dense length.  The parts of the holes below J are the
// destinations; the filled stretches above J (between consecutive holes) are the sources; both
// lists are in position order, and slot t of one is paired with slot t of the other (the reference
// pairs the lowest holes with the HIGHEST tuples, npj.cpp:486-511: same set of rows in [0, J), and
// the order of a join result is unspecified).  Two prefix sums and, per hole, a binary search in
// the sources' prefix give the moves; a first pass counts them, a second writes them.
// (The two-pointer walk by one thread took 1.5 of close_gaps' 1.8 ms at 4096 workers.)
__global__ __launch_bounds__(CG_BLOCK) void close_gaps_plan_kernel(
    const u64 *__restrict__ final_offsets, uint32_t nworkers, u64 block_size,
    const u64 *__restrict__ block_counter, const uint32_t *__restrict__ overflow,
    Move *moves, uint32_t *nmoves, u64 *dense_count)
{
    // an overflowed join left cursors that do not describe disjoint holes: plan nothing
    if (*overflow) {
        if (threadIdx.x == 0) { hj_store(nmoves, 0u); hj_store(dense_count, (u64)0); }
        return;
    }
    __shared__ u64 hole_beg[CG_MAX];            // sorted hole starts, then prefix of the destination sizes
    __shared__ u64 hole_end[CG_MAX];            // prefix of the source sizes
    __shared__ u64 scratch[CG_BLOCK / 64 + 1];
    __shared__ u64 sh_count, sh_top, sh_holes;
    const int tid = threadIdx.x;
    uint32_t N = 64;                            // sort size: next power of two >= nworkers
    while (N < nworkers) N <<= 1;
    // holes with no cursor sort to the end (key = ~0)
    for (uint32_t i = tid; i < N; i += CG_BLOCK)
        hole_beg[i] = (i < nworkers) ? final_offsets[i] : HJ_NO_CURSOR;
    __syncthreads();
    for (uint32_t size = 2; size <= N; size <<= 1) {
        for (uint32_t strd = size >> 1; strd > 0; strd >>= 1) {
            for (uint32_t i = tid; i < N / 2; i += CG_BLOCK) {
                const uint32_t lo = 2 * i - (i & (strd - 1));
                const uint32_t hi = lo + strd;
                const bool up = ((lo & size) == 0);
                const u64 x = hole_beg[lo], y = hole_beg[hi];
                if ((x > y) == up) { hole_beg[lo] = y; hole_beg[hi] = x; }
            }
            __syncthreads();
        }
    }
    // number of real holes, top, total hole size (each thread owns the elements i = tid * per + j)
    const uint32_t per = (N + CG_BLOCK - 1) / CG_BLOCK;
    const uint32_t lo = min(N, (uint32_t)tid * per), hi = min(N, lo + per);
    auto end_of = [&](u64 b) -> u64 { return (b & ~(block_size - 1)) + block_size; };
    {
        u64 cnt = 0, holes = 0, top = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const u64 b = hole_beg[i];
            if (b != HJ_NO_CURSOR) { ++cnt; holes += end_of(b) - b; top = max(top, end_of(b)); }
        }
        if (tid == 0) { sh_count = 0; sh_top = 0; sh_holes = 0; }
        __syncthreads();
        if (cnt) { atomicAdd(&sh_count, cnt); atomicAdd(&sh_holes, holes); atomicMax(&sh_top, top); }
        __syncthreads();
    }
    const uint32_t count = (uint32_t)sh_count;
    const u64 top = sh_top, J = top - sh_holes;
    if (count == 0) {
        if (tid == 0) { hj_store(nmoves, 0u); hj_store(dense_count, (u64)0); }
        return;
    }
    // destination part of hole i: [b_i, min(e_i, J)); source stretch i: [max(e_{i-1}, J), b_i), i >= 1
    u64 dsz[CG_MAX / CG_BLOCK], ssz[CG_MAX / CG_BLOCK], sb[CG_MAX / CG_BLOCK], db[CG_MAX / CG_BLOCK];
    u64 dsum = 0, ssum = 0;
    for (uint32_t i = lo, j = 0; i < hi; ++i, ++j) {
        dsz[j] = ssz[j] = sb[j] = db[j] = 0;
        if (i < count) {
            const u64 b = hole_beg[i], e = end_of(b);
            db[j] = b;
            if (b < J) dsz[j] = min(e, J) - b;
            const u64 from = max(i > 0 ? end_of(hole_beg[i - 1]) : 0ull, J);    // filled from here up to the hole
            if (b > from) { sb[j] = from; ssz[j] = b - from; }
            dsum += dsz[j]; ssum += ssz[j];
        }
    }
    __syncthreads();                             // everybody has read its neighbours' hole_beg
    u64 drun = block_exclusive_scan<CG_BLOCK, u64>(dsum, scratch);
    __syncthreads();
    u64 srun = block_exclusive_scan<CG_BLOCK, u64>(ssum, scratch);
    // the sorted starts are no longer needed in LDS: hole_beg := prefix of the destination sizes,
    // hole_end := prefix of the source sizes (the end of the last stretch is never needed)
    __syncthreads();
    for (uint32_t i = lo, j = 0; i < hi; ++i, ++j) {
        hole_beg[i] = drun; hole_end[i] = srun;
        drun += dsz[j]; srun += ssz[j];
    }
    __syncthreads();
    // hole i's destination slots are [D_i, D_i + dsz_i); source stretch s covers slots [S_s, S_s + ssz_s).
    // Count the moves of my holes: one per source stretch that overlaps the hole's slot interval.
    auto first_stretch = [&](u64 t) -> uint32_t {          // largest s with S_s <= t (stretches of size 0 share a prefix)
        uint32_t a = 0, b = count;
        while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (hole_end[m] <= t) a = m; else b = m; }
        return a;
    };
    // the stretches' start positions are needed by other threads and LDS is full: global scratch
    // behind the move list (same workgroup, read after a barrier)
    u64 *stretch_beg = reinterpret_cast<u64 *>(moves + 2 * HJ_MAX_WORKERS);
    for (uint32_t i = lo, j = 0; i < hi; ++i, ++j) if (i < count) hj_store(&stretch_beg[i], sb[j]);
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = lo, j = 0; i < hi; ++i, ++j) {
        if (i >= count || dsz[j] == 0) continue;
        const u64 t0 = hole_beg[i], t1 = t0 + dsz[j];
        uint32_t s = first_stretch(t0);
        while (s < count) {
            const u64 s0 = hole_end[s], s1 = (s + 1 < count) ? hole_end[s + 1] : ~0ull;
            if (s0 >= t1) break;
            if (s1 > t0 && s1 > s0) ++mine;
            ++s;
        }
    }
    __syncthreads();
    const u64 mbase = block_exclusive_scan<CG_BLOCK, u64>((u64)mine, scratch);
    uint32_t at = (uint32_t)mbase;
    for (uint32_t i = lo, j = 0; i < hi; ++i, ++j) {
        if (i >= count || dsz[j] == 0) continue;
        const u64 t0 = hole_beg[i], t1 = t0 + dsz[j];
        uint32_t s = first_stretch(t0);
        while (s < count) {
            const u64 s0 = hole_end[s], s1 = (s + 1 < count) ? hole_end[s + 1] : ~0ull;
            if (s0 >= t1) break;
            if (s1 > t0 && s1 > s0) {
                const u64 a0 = max(t0, s0), a1 = min(t1, s1);       // overlapping slots
                hj_store(&moves[at].dst, db[j] + (a0 - t0));
                hj_store(&moves[at].src, stretch_beg[s] + (a0 - s0));
                hj_store(&moves[at].cnt, a1 - a0);
                ++at;
            }
            ++s;
        }
    }
    if (tid == CG_BLOCK - 1) hj_store(nmoves, (uint32_t)(mbase + mine));
    if (tid == 0) hj_store(dense_count, J);
}

// The whole chip copies the planned moves: one move per workgroup at a time
// (sources lie above every remaining hole, so a move never overlaps its
// destination or another move; a move is at most one block long).
__global__ __launch_bounds__(256) void close_gaps_copy_kernel(
    uint32_t *k, uint32_t *ov, uint32_t *iv, const Move *__restrict__ moves,
    const uint32_t *__restrict__ nmoves)
{
    const uint32_t nm = *nmoves;
    for (uint32_t m = blockIdx.x; m < nm; m += gridDim.x) {
        const u64 dst = moves[m].dst, src = moves[m].src, cnt = moves[m].cnt;
        for (u64 i = threadIdx.x; i < cnt; i += 256) {
            // (non-temporal like the rows themselves: a move that is lost leaves a hole's stale row inside the dense result)
            hj_store(&k[dst + i], k[src + i]);
            hj_store(&ov[dst + i], ov[src + i]);
            if (iv) hj_store(&iv[dst + i], iv[src + i]);         // (semi- / anti-joins: no inner_val column)
        }
    }
}

int hj_launch_close_gaps_ex(uint32_t *k, uint32_t *ov, uint32_t *iv, const u64 *final_offsets,
                            uint32_t nworkers, u64 block_size, const u64 *block_counter,
                            const uint32_t *overflow, void *moves, uint32_t *nmoves,
                            u64 *dense_count, int cus, hipStream_t stream)
{
    if (nworkers > CG_MAX) return HJGPU_EINVAL;
    hipLaunchKernelGGL(close_gaps_plan_kernel, dim3(1), dim3(CG_BLOCK), 0, stream,
                       final_offsets, nworkers, block_size, block_counter, overflow,
                       reinterpret_cast<Move *>(moves), nmoves, dense_count);
    hipLaunchKernelGGL(close_gaps_copy_kernel, dim3(cus * 4), dim3(256), 0, stream, k, ov, iv,
                       reinterpret_cast<const Move *>(moves), nmoves);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}
