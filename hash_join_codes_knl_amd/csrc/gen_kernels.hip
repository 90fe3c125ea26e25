// gen_kernels.hip — counter-based relation generator and column checksums.
//
// Statistical contract of the reference generator (generate_data_for_join,
// cpra2.cpp:1578-1696; write.cpp:1482-1646): unique non-zero build keys, probe
// keys drawn from the build keys (each build key at least once when
// outer >= inner, the rest uniform picks), payload = key * odd factor, both
// columns in pseudo-random order.  The reference builds this with a serial
// MT19937 stream, a CAS hash set and a Fisher-Yates shuffle; here every tuple
// is a pure function of (seed, position), so any shard of the probe side can
// be generated independently on its own GPU with no communication
// (SURVEY.md §8f row 1).  Bit-compatibility with the MT19937 stream is NOT a
// goal (the host-side oracle generator covers that, oracle/hj_oracle.c).
#include "hj_device.hpp"
#include "hj_internal.hpp"
#include "hj_lookup.hpp"
#include "hj_emit.hpp"
#include <algorithm>
#include <math.h>

// lowbias32: a bijection on 32-bit integers with mix32(0) == 0, hence
// mix32(x) != 0 for x != 0 and distinct x give distinct keys.
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ u64 splitmix64(u64 z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct GenArgs {
    u64 seed;
    u64 inner, inner_begin, inner_count, outer_total, outer_begin, outer_count;
    u64 distinct;               // min(inner, outer_total)  (write.cpp:1687-1689)
    u64 mul, add;               // position permutation j' = (j*mul + add) mod outer_total
    u64 mul_r, add_r;           // same for the build side, mod inner
    uint32_t key_base;          // build key i = mix32(key_base + i), key_base + i in [1, 2^32)
    uint32_t inner_factor, outer_factor;
    double zipf;                // > 0: repeat picks of the probe side follow a Zipf law over the distinct keys
    double zipf_a, zipf_b;      // rank = (a*x + 1)^b for x uniform in (0,1)   (s != 1);  distinct^x  (s == 1)
    // selectivity (write.cpp:1685-1689): the build side draws from unique[0, d), the probe side from
    // unique[d - join_d, 2d - join_d): probe rank r is build rank d - join_d + r, a match iff r < join_d
    u64 join_d, outer_shift;    // outer_shift = d - join_d
    u64 *expect;                // device [4] or NULL: count, sum key, sum key * outer_factor, sum key * inner_factor of the matching probe tuples
    uint32_t *ik, *iv, *ok, *ov;
};

__global__ __launch_bounds__(256) void generate_kernel(GenArgs a)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.ik) {
        for (u64 j = tid; j < a.inner_count; j += stride) {
            const u64 i = a.inner_begin + j;
            const u64 ip = (i * a.mul_r + a.add_r) % a.inner;
            u64 r;
            if (ip < a.distinct) r = ip;                               // every distinct key once
            else r = __umul64hi(splitmix64(ip ^ ~a.seed), a.distinct); // then repeats (outer < inner)
            const uint32_t k = mix32(a.key_base + (uint32_t)r);
            hj_store(&a.ik[j], k);
            hj_store(&a.iv[j], k * a.inner_factor);
        }
    }
    if (a.ok) {
        u64 e_n = 0, e_k = 0, e_o = 0, e_i = 0;
        for (u64 j = tid; j < a.outer_count; j += stride) {
            const u64 pos = a.outer_begin + j;
            const u64 jp = (pos * a.mul + a.add) % a.outer_total;     // "shuffle": a bijection of positions
            u64 r;
            if (jp < a.distinct) r = jp;                               // every distinct key once
            else if (a.zipf > 0.0) {
                // continuous inverse-CDF approximation of a Zipf(s) law over ranks 1..distinct
                // (the same formula as the host generator, host/write_main.cpp; write.cpp:1477-1480
                // is the reference's unfinished attempt): rank 1 is the hottest key
                const double x = ((double)(splitmix64(jp ^ a.seed) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
                const double rank = a.zipf_b == 0.0 ? pow((double)a.distinct, x) : pow(a.zipf_a * x + 1.0, a.zipf_b);
                r = rank >= 1.0 ? (u64)rank - 1 : 0;
                if (r >= a.distinct) r = a.distinct - 1;
            } else r = __umul64hi(splitmix64(jp ^ a.seed), a.distinct);  // then uniform picks
            const uint32_t k = mix32(a.key_base + (uint32_t)(a.outer_shift + r));
            hj_store(&a.ok[j], k);
            hj_store(&a.ov[j], k * a.outer_factor);
            if (r < a.join_d) { e_n += 1; e_k += k; e_o += (uint32_t)(k * a.outer_factor); e_i += (uint32_t)(k * a.inner_factor); }
        }
        if (a.expect) {
            // the aggregates the join of this probe range with the (unique-key) build side must return
            e_n = wave_reduce_sum(e_n); e_k = wave_reduce_sum(e_k); e_o = wave_reduce_sum(e_o); e_i = wave_reduce_sum(e_i);
            if (hj_lane() == 0 && e_n) {
                atomicAdd(&a.expect[0], e_n); atomicAdd(&a.expect[1], e_k);
                atomicAdd(&a.expect[2], e_o); atomicAdd(&a.expect[3], e_i);
            }
        }
    }
}

static u64 gcd_u64(u64 x, u64 y) { while (y) { u64 t = x % y; x = y; y = t; } return x; }

int hj_launch_generate(u64 seed, size_t inner, size_t inner_begin, size_t inner_count,
                       size_t outer_total, size_t outer_begin,
                       size_t outer_count, uint32_t inner_factor, uint32_t outer_factor,
                       uint32_t *ik, uint32_t *iv, uint32_t *ok, uint32_t *ov, hipStream_t stream, double zipf,
                       double selectivity, u64 *d_expect)
{
    if (!(selectivity >= 0.0) || selectivity > 1.0) return HJGPU_EINVAL;
    if (inner == 0 || inner >= 0xFFFFFFFFull) return HJGPU_EINVAL;
    if (ik && inner_begin + inner_count > inner) return HJGPU_EINVAL;
    if (ok && (outer_total == 0 || outer_begin + outer_count > outer_total)) return HJGPU_EINVAL;
    if (outer_total >= (1ull << 35)) return HJGPU_EINVAL;      // pos*mul must stay below 2^64
    GenArgs a;
    a.seed = seed * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull;
    a.inner = inner; a.inner_begin = inner_begin; a.inner_count = inner_count;
    a.outer_total = outer_total ? outer_total : 1;
    a.outer_begin = outer_begin; a.outer_count = outer_count;
    u64 mul = 402653189ull;                                    // prime < 2^29
    while (gcd_u64(mul, a.outer_total) != 1) mul += 2;
    a.mul = mul;
    u64 mul_r = 268435459ull;                                  // prime > 2^28
    while (gcd_u64(mul_r, (u64)inner) != 1) mul_r += 2;
    a.mul_r = mul_r;
    a.add_r = (a.seed >> 13) % inner;
    a.distinct = (outer_total && outer_total < inner) ? outer_total : inner;
    a.add = (a.seed >> 7) % a.outer_total;
    a.join_d = (u64)((double)a.distinct * selectivity);           // write.cpp:1689
    if (a.join_d > a.distinct) a.join_d = a.distinct;
    a.outer_shift = a.distinct - a.join_d;
    a.expect = d_expect;
    if (2 * a.distinct - a.join_d >= 0xFFFFFFFFull) return HJGPU_EINVAL;
    a.key_base = 1u + (uint32_t)((a.seed >> 11) % (0xFFFFFFFFull - (2 * a.distinct - a.join_d)));
    a.inner_factor = inner_factor | 1u; a.outer_factor = outer_factor | 1u;
    a.zipf = zipf > 0.0 ? zipf : 0.0; a.zipf_a = a.zipf_b = 0.0;
    if (a.zipf > 0.0 && fabs(a.zipf - 1.0) >= 1e-9) {
        a.zipf_a = pow((double)a.distinct, 1.0 - a.zipf) - 1.0;
        a.zipf_b = 1.0 / (1.0 - a.zipf);
    }
    a.ik = ik; a.iv = iv; a.ok = ok; a.ov = ov;
    hipLaunchKernelGGL(generate_kernel, dim3(4096), dim3(256), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// sums[0] += key, sums[1] += key*fa, sums[2] += key*fb  (products mod 2^32)
// Also the "simple dwordx4 read kernel" of SURVEY 8d: 16-byte loads, 4 per lane in flight,
// nothing written - bench.py times it for the empirical streaming-read ceiling of the box.
__global__ __launch_bounds__(256) void column_sums_kernel(const uint32_t *__restrict__ keys, u64 n,
                                                          uint32_t fa, uint32_t fb, u64 *sums)
{
    __shared__ u64 red[3][4];
    u64 s0 = 0, s1 = 0, s2 = 0;
    auto add = [&](uint32_t k) { s0 += k; s1 += (uint32_t)(k * fa); s2 += (uint32_t)(k * fb); };
    const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    // scalar head up to the first 16-byte boundary, vector body, scalar tail
    const u64 head = min(n, (u64)((16 - ((uintptr_t)keys & 15)) & 15) / 4);
    const uint4 *v = (const uint4 *)(keys + head);
    const u64 nv = (n - head) / 4;
    u64 i = tid;
    for (; i + 3 * stride < nv; i += 4 * stride) {
        const uint4 a = v[i], b = v[i + stride], c = v[i + 2 * stride], d = v[i + 3 * stride];
        add(a.x); add(a.y); add(a.z); add(a.w); add(b.x); add(b.y); add(b.z); add(b.w);
        add(c.x); add(c.y); add(c.z); add(c.w); add(d.x); add(d.y); add(d.z); add(d.w);
    }
    for (; i < nv; i += stride) { const uint4 a = v[i]; add(a.x); add(a.y); add(a.z); add(a.w); }
    if (tid < head) add(keys[tid]);
    const u64 done = head + nv * 4;
    if (tid < n - done) add(keys[done + tid]);
    s0 = wave_reduce_sum(s0); s1 = wave_reduce_sum(s1); s2 = wave_reduce_sum(s2);
    const int wave = threadIdx.x >> 6;
    if (hj_lane() == 0) { red[0][wave] = s0; red[1][wave] = s1; red[2][wave] = s2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        u64 s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        atomicAdd(&sums[threadIdx.x], s);
    }
}

int hj_launch_column_sums(const uint32_t *keys, size_t n, uint32_t fa, uint32_t fb, u64 *sums3,
                          hipStream_t stream)
{
    if (hj_zero_async(sums3, 3 * sizeof(u64), stream) != hipSuccess) return HJGPU_EHIP;
    hipLaunchKernelGGL(column_sums_kernel, dim3(2048), dim3(256), 0, stream, keys, (u64)n, fa, fb, sums3);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// The "simple dwordx4 read kernel" of SURVEY 8d: 1024-thread workgroups sweep 64 KiB pieces, four
// 16-byte loads per lane in flight, the data only XORed together (column_sums_kernel's two 32-bit
// multiplies per key make IT instruction-bound at ~5.2 TB/s; this one reads at 6.6-6.7 TB/s).
__global__ __launch_bounds__(1024) void stream_read_kernel(const uint4 *__restrict__ in, u64 pieces, uint4 *sink)
{
    uint4 acc = make_uint4(0, 0, 0, 0);
    for (u64 t = blockIdx.x; t < pieces; t += gridDim.x) {
        const uint4 *p = in + t * 4096 + threadIdx.x;
        const uint4 a = p[0], b = p[1024], c = p[2048], d = p[3072];
        acc.x ^= a.x ^ b.y; acc.y ^= c.z ^ d.w; acc.z ^= a.z ^ c.x; acc.w ^= b.w ^ d.y;
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9E3779B9u) hj_store(sink, acc);      // keeps the loads alive
}

int hj_launch_stream_read(const void *p, size_t bytes, void *sink16, int cus, hipStream_t stream)
{
    const u64 pieces = bytes / 65536;
    if (pieces == 0 || ((uintptr_t)p & 15)) return HJGPU_EINVAL;
    hipLaunchKernelGGL(stream_read_kernel, dim3(cus * 2), dim3(1024), 0, stream, (const uint4 *)p, pieces, (uint4 *)sink16);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// Random 64-byte line reads (hjgpu_random_line_read_ms): the access shape of the NPJ probe without the join - the four
// lanes of a quad fetch the four quarters of one pseudo-random line of the buffer with ONE load instruction, four lines
// in flight per quad.  What it reaches is the memory system's rate for independent 64-byte reads out of a table that
// does not fit the caches (requests per second, not bytes, are the limit: profiles/r03_request_size.txt), i.e. the ceiling bench.py prices NPJ against.
__global__ __launch_bounds__(256) void random_line_read_kernel(const uint4 *__restrict__ in, u64 lines, u64 reads, uint4 *sink)
{
    uint4 acc = make_uint4(0, 0, 0, 0);
    const uint32_t sub = threadIdx.x & 3;
    const u64 quads = (u64)gridDim.x * 64, quad = (u64)blockIdx.x * 64 + (threadIdx.x >> 2);
    for (u64 r = quad * 4; r < reads; r += quads * 4) {
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // a multiplicative hash of the read's index, as the join's H(key, f, lines)
            const u64 x = (u64)(uint32_t)((uint32_t)(r + i) * 0x9E3779B1u) ^ ((r + i) >> 32);
            const u64 line = (u64)(((unsigned __int128)(x & 0xFFFFFFFFull) * lines) >> 32);
            v[i] = in[4 * line + sub];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { acc.x ^= v[i].x; acc.y ^= v[i].y; acc.z ^= v[i].z; acc.w ^= v[i].w; }
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9E3779B9u) hj_store(sink, acc);      // keeps the loads alive
}

int hj_launch_random_line_read(const void *p, size_t bytes, size_t reads, void *sink16, int cus, hipStream_t stream)
{
    const u64 lines = bytes / 64;
    if (lines == 0 || reads == 0 || ((uintptr_t)p & 63)) return HJGPU_EINVAL;
    hipLaunchKernelGGL(random_line_read_kernel, dim3(cus * 8), dim3(256), 0, stream, (const uint4 *)p, lines, (u64)reads, (uint4 *)sink16);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// Random 8-byte compare-and-swaps (hjgpu_random_cas_ms): the access shape of the NPJ build (npj.cpp:196-210: one CAS of an
// empty bucket per build tuple) without the join - `ops` independent pseudo-random buckets of a zeroed buffer, each claimed
// with ONE 64-bit CAS (expected 0), U of them in flight per lane; LOAD: a plain load of the bucket first, as the build
// does to skip taken buckets.  What it reaches is the memory system's rate for independent returning atomics.
template <int U, bool LOAD>
__global__ __launch_bounds__(256) void random_cas_kernel(u64 *__restrict__ table, u64 buckets, u64 ops, u64 *sink)
{
    u64 acc = 0;
    const u64 stride = (u64)gridDim.x * 256 * U;
    for (u64 r = ((u64)blockIdx.x * 256 + threadIdx.x) * U; r < ops; r += stride) {
        u64 at[U], seen[U], old[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const u64 x = (u64)(uint32_t)((uint32_t)(r + i) * 0x9E3779B1u) ^ ((r + i) >> 32);
            at[i] = (u64)(((unsigned __int128)(x & 0xFFFFFFFFull) * buckets) >> 32);
            seen[i] = 0;
        }
        if (LOAD) {
#pragma unroll
            for (int i = 0; i < U; ++i) seen[i] = __builtin_nontemporal_load(&table[at[i]]);
        }
        // all U atomics are issued back to back (no predicate around them: an operation past `ops` or on a bucket that was
        // seen taken compares with a value no bucket holds and changes nothing)
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const bool live = r + i < ops && (uint32_t)seen[i] == 0u;
            old[i] = atomicCAS(&table[at[i]], live ? 0ull : ~0ull, live ? (((r + i) << 1) | 1ull) : ~0ull);
        }
#pragma unroll
        for (int i = 0; i < U; ++i) acc ^= old[i];
    }
    if (acc == 0x9E3779B97F4A7C15ull) *sink = acc;          // keeps the returns alive
}

int hj_launch_random_cas(void *p, size_t bytes, size_t ops, int in_flight, bool load_first, void *sink8, int cus, hipStream_t stream)
{
    const u64 buckets = bytes / 8;
    if (buckets == 0 || ops == 0 || ((uintptr_t)p & 7)) return HJGPU_EINVAL;
    u64 *t = (u64 *)p, *sk = (u64 *)sink8;
    const dim3 grid(cus * 16), block(256);
#define RC(U, L) hipLaunchKernelGGL((random_cas_kernel<U, L>), grid, block, 0, stream, t, buckets, (u64)ops, sk)
    if (in_flight == 1) { if (load_first) RC(1, true); else RC(1, false); }
    else if (in_flight == 2) { if (load_first) RC(2, true); else RC(2, false); }
    else if (in_flight == 4) { if (load_first) RC(4, true); else RC(4, false); }
    else if (in_flight == 8) { if (load_first) RC(8, true); else RC(8, false); }
    else return HJGPU_EINVAL;
#undef RC
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// Placement probe (hjgpu_api.hip, ensure_placed): a plain streaming fill of a freshly allocated buffer.  Its rate
// differs by up to 26 % between allocations of the same size on one MI355X (physical placement; profiles/r02_placement.txt)
// and predicts how fast K6 pass 1 will write into that buffer.
__global__ __launch_bounds__(1024) void fill_probe_kernel(uint4 *__restrict__ out, u64 n)
{
    const uint4 v = make_uint4(0, 0, 0, 0);
    for (u64 i = (u64)blockIdx.x * 1024 + threadIdx.x; i < n; i += (u64)gridDim.x * 1024) out[i] = v;
}

// Result rows -> page-locked host memory by a KERNEL (16-byte stores over PCIe; few workgroups: the bus, not the CUs, is the
// limit).  hjgpu_join_host_rows sends a batch's rows home while the next batch is uploaded: with hipMemcpyAsync in both
// directions the runtime put upload and download on the same DMA engine from the second call of a process on (one after
// the other: 430 ms instead of 255 for 8.5 GB up and 12 GB down); the DMA engines now carry the upload only.
__global__ __launch_bounds__(256) void copy_to_host_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, u64 n)
{
    // 32-bit elements (a batch's rows start wherever the batches before it ended): a wave's store is 256 contiguous bytes
    const u64 stride = (u64)gridDim.x * 256;
    u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    for (; i + 7 * stride < n; i += 8 * stride) {
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[i + j * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) hj_store(&dst[i + j * stride], v[j]);
    }
    for (; i < n; i += stride) hj_store(&dst[i], src[i]);
}

int hj_launch_copy_to_host(void *host_mapped, const void *d, size_t bytes, hipStream_t stream)
{
    if (!bytes) return HJGPU_OK;
    if (((uintptr_t)host_mapped & 3) || ((uintptr_t)d & 3) || (bytes & 3)) return HJGPU_EALIGN;
    hipLaunchKernelGGL(copy_to_host_kernel, dim3(64), dim3(256), 0, stream, (uint32_t *)host_mapped, (const uint32_t *)d, (u64)(bytes / 4));
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// Clears and device-to-device copies of the library's own state and of the caller's columns: own kernels, because the runtime's
// (hipMemsetAsync, hipMemcpyAsync) store plainly and the library's store policy (hj_device.hpp) has no plain store beside other
// queues' work - NPJ's 2 GB table clear writes as many bytes as a K6 pass over the build side.  Any 4-byte aligned range; the
// body in 16-byte non-temporal stores.
__global__ __launch_bounds__(256) void zero_kernel(uint32_t *__restrict__ p, u64 words, uint32_t word)
{
    // words [0, head) up to the first 16-byte boundary, 16-byte vectors, then the tail
    const u64 head = min(words, (u64)((16 - ((uintptr_t)p & 15)) & 15) / 4);
    const u64 vecs = (words - head) / 4, tail0 = head + vecs * 4;
    uint4 *v = reinterpret_cast<uint4 *>(p + head);
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, stride = (u64)gridDim.x * 256;
    for (u64 i = tid; i < vecs; i += stride) hj_store(&v[i], make_uint4(word, word, word, word));
    if (tid < head) hj_store(&p[tid], word);
    if (tid < words - tail0) hj_store(&p[tail0 + tid], word);
}

__global__ __launch_bounds__(256) void copy_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, u64 words, uint32_t vec)
{
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, stride = (u64)gridDim.x * 256;
    if (vec) {              // both 16-byte aligned: 4 vectors in flight per lane
        const u64 vecs = words / 4;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        u64 i = tid;
        for (; i + 3 * stride < vecs; i += 4 * stride) {
            const uint4 a = hj_load_nt(s4 + i), b = hj_load_nt(s4 + i + stride), c = hj_load_nt(s4 + i + 2 * stride), d = hj_load_nt(s4 + i + 3 * stride);
            hj_store(&d4[i], a); hj_store(&d4[i + stride], b); hj_store(&d4[i + 2 * stride], c); hj_store(&d4[i + 3 * stride], d);
        }
        for (; i < vecs; i += stride) hj_store(&d4[i], hj_load_nt(s4 + i));
        if (tid < words - vecs * 4) hj_store(&dst[vecs * 4 + tid], src[vecs * 4 + tid]);
    } else
        for (u64 i = tid; i < words; i += stride) hj_store(&dst[i], src[i]);
}

hipError_t hj_fill_async(void *p, uint32_t word, size_t bytes, hipStream_t stream)
{
    if (!bytes) return hipSuccess;
    if (((uintptr_t)p & 3) || (bytes & 3)) return word == 0 ? hipMemsetAsync(p, 0, bytes, stream) : hipErrorInvalidValue;      // (no such caller: every clear is of 4-byte words)
    const u64 words = bytes / 4;
    const unsigned grid = (unsigned)std::min<u64>((words / 4 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(zero_kernel, dim3(grid), dim3(256), 0, stream, (uint32_t *)p, words, word);
    return hipGetLastError();
}

hipError_t hj_zero_async(void *p, size_t bytes, hipStream_t stream) { return hj_fill_async(p, 0u, bytes, stream); }

hipError_t hj_copy_async(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    if (!bytes) return hipSuccess;
    if (((uintptr_t)dst & 3) || ((uintptr_t)src & 3) || (bytes & 3)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream);
    const u64 words = bytes / 4;
    const uint32_t vec = (((uintptr_t)dst | (uintptr_t)src) & 15) == 0 ? 1u : 0u;
    const unsigned grid = (unsigned)std::min<u64>((words / (vec ? 16 : 1) + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, stream, (uint32_t *)dst, (const uint32_t *)src, words, vec);
    return hipGetLastError();
}

int hj_launch_fill_probe(void *p, size_t bytes, hipStream_t stream)
{
    if (((uintptr_t)p & 15) || bytes < 16) return HJGPU_EINVAL;
    hipLaunchKernelGGL(fill_probe_kernel, dim3(1024), dim3(1024), 0, stream, (uint4 *)p, (u64)(bytes / 16));
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// ---- compaction by bitmap (hjgpu_compact_selected; DESIGN.md section 5 "Compaction by bitmap") ----------------------------------------
// Two launches, ordered by the stream; no workgroup ever waits for another.  Both have one workgroup per range of compact_layout.hpp.
// Launch 1: workgroup g counts the set bits of its range's mask words, counts[g].  16-byte non-temporal loads while whole vectors lie inside
// the range's whole words, single words behind them: nothing at or beyond word (n + 31) / 32 is read; the last word's bits at n and beyond do
// not count.  An empty range stores 0.
__global__ __launch_bounds__(256) void compact_count_kernel(const uint32_t *__restrict__ select_bits, hj_compact::Layout lay, u64 *counts)
{
    __shared__ u64 red[4];
    const u64 rb = lay.begin(blockIdx.x), re = lay.end(blockIdx.x);
    u64 c = 0;
    if (re > rb) {
        const u64 w0 = rb >> 5, w1 = (re + 31) >> 5;                    // rb is a multiple of 256 rows: word w0 is 16-byte aligned
        const u64 vecs = ((re >> 5) - w0) >> 2;                        // whole vectors of whole words: a partial last word is never among them
        const uint4 *v4 = reinterpret_cast<const uint4 *>(select_bits + w0);
        u64 i = threadIdx.x;
        uint32_t s = 0;
        for (; i + 768 < vecs; i += 1024) {
            const uint4 a = hj_load_nt(v4 + i), b = hj_load_nt(v4 + i + 256), d = hj_load_nt(v4 + i + 512), e = hj_load_nt(v4 + i + 768);
            s += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
            s += __popc(d.x) + __popc(d.y) + __popc(d.z) + __popc(d.w) + __popc(e.x) + __popc(e.y) + __popc(e.z) + __popc(e.w);
            c += s; s = 0;
        }
        for (; i < vecs; i += 256) { const uint4 a = hj_load_nt(v4 + i); s += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w); }
        // the words behind the last whole vector (at most 4), the range's last word cut at its last row
        const u64 w = w0 + vecs * 4 + threadIdx.x;
        if (w < w1) {
            uint32_t x = hj_load_nt(select_bits + w);
            if (w == w1 - 1 && (re & 31)) x &= (1u << (uint32_t)(re & 31)) - 1u;
            s += __popc(x);
        }
        c += s;
    }
    c = wave_reduce_sum(c);
    if (hj_lane() == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) hj_store(&counts[blockIdx.x], red[0] + red[1] + red[2] + red[3]);
}

// The count alone (ncols == 0 and no row numbers): *d_count = the sum of counts[0 .. ranges)
__global__ __launch_bounds__(256) void compact_total_kernel(const u64 *__restrict__ counts, uint32_t ranges, u64 *d_count)
{
    __shared__ u64 red[4];
    u64 s = 0;
    for (uint32_t t = threadIdx.x; t < ranges; t += 256) s += counts[t];
    s = wave_reduce_sum(s);
    if (hj_lane() == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) hj_store(d_count, red[0] + red[1] + red[2] + red[3]);
}

// orders this wave's LDS traffic for the compiler (the hardware performs a wave's LDS instructions in the order they were issued)
__device__ __forceinline__ void compact_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t compact_elem(const uint4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// Launch 2: workgroup g adds up counts[0 .. g) - where its range's first survivor goes; workgroup 0 adds up all of them and stores *d_count -
// and walks its range chunk by chunk.  Wave w owns the chunk's rows [w * VEC * 256, (w + 1) * VEC * 256) in VEC trips of hj_lookup.hpp's
// layout: lane L owns rows 4 L ... 4 L + 3 of a trip, a group of 8 lanes one mask word and one 128-byte line of every column.  The mask
// words of all trips are loaded first, then the columns; a group whose word is 0 loads no column; a row at n or beyond is never selected
// (lookup_fetch's nibble), and the last, partial vector of a column is loaded by words: nothing at row n or beyond is read.  popcount per lane ->
// prefix over the wave (DPP) -> the four waves' totals through LDS, one LDS-only barrier per chunk (the totals alternate between two slots:
// a wave that is a chunk ahead writes the other one).  The output is in input order whatever the grid.
// STAGED: a wave's survivors of one column go to the wave's own piece of LDS in output order and leave as 4-byte stores of 64 consecutive
// lanes, 256 contiguous bytes per instruction; else every lane stores its own rows (up to four 4-byte stores, dense across the workgroup).
// Rows whose output index is capacity or beyond are not stored.  NCOLS, ROWS and STAGED are template parameters: no store behind a run-time flag.
template <int NCOLS, bool ROWS, bool STAGED>
__global__ __launch_bounds__(256) void compact_kernel(CompactArgs a)
{
    constexpr int VEC = hj_compact::VEC;
    constexpr int WAVE_ROWS = VEC * 256;
    __shared__ u64 red[4];
    __shared__ __attribute__((aligned(16))) uint32_t tot[2][4];
    __shared__ uint32_t stage[STAGED ? 4 : 1][STAGED ? WAVE_ROWS : 1];
    const uint32_t g = blockIdx.x, wave = threadIdx.x >> 6, lane = hj_lane();
    u64 s = 0;
    const uint32_t lim = g ? g : a.lay.ranges;
    for (uint32_t t = threadIdx.x; t < lim; t += 256) s += a.counts[t];
    s = wave_reduce_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = red[0] + red[1] + red[2] + red[3];
    if (g == 0 && a.d_count && threadIdx.x == 0) hj_store(a.d_count, s);
    u64 run = g ? hj_uniform(s) : 0;                                   // output index of the chunk's first survivor
    const u64 n = a.lay.n, rb = a.lay.begin(g), re = a.lay.end(g), nvec = (n + 3) >> 2;
    uint32_t par = 0;
    for (u64 row0 = rb; row0 < re; row0 += hj_compact::CHUNK_ROWS, par ^= 1u) {
        const u64 v0 = (row0 >> 2) + (u64)wave * (VEC * 64) + lane;
        uint32_t w[VEC], nib[VEC];
        uint4 kk[NCOLS ? NCOLS : 1][VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const u64 v = v0 + (u64)u * 64;
            w[u] = 0;
            if (v < nvec) w[u] = hj_load_nt(a.select_bits + (v >> 3));   // (v < nvec: row 4 v < n, and word v / 8 starts at or before it)
        }
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const u64 v = v0 + (u64)u * 64, r0 = v << 2;
            const uint32_t rows = r0 + 4 <= n ? 15u : r0 < n ? (1u << (uint32_t)(n - r0)) - 1u : 0u;
            nib[u] = (w[u] >> ((threadIdx.x & 7u) * 4)) & rows;
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) {
                kk[c][u] = make_uint4(0, 0, 0, 0);
                if (w[u] != 0u) {                                        // (w != 0 only where v < nvec)
                    if (rows == 15u) kk[c][u] = hj_load_nt(reinterpret_cast<const uint4 *>(a.in[c]) + v);
                    else {                                               // the column's last, partial vector
                        if (rows & 1u) kk[c][u].x = hj_load_nt(a.in[c] + r0);
                        if (rows & 2u) kk[c][u].y = hj_load_nt(a.in[c] + r0 + 1);
                        if (rows & 4u) kk[c][u].z = hj_load_nt(a.in[c] + r0 + 2);
                    }
                }
            }
        }
        // where this lane's survivors go: [loc[u], loc[u] + popcount(nib[u])) of the wave's, the wave's from `before` of the chunk's
        uint32_t loc[VEC], wtotal = 0;
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const uint32_t cnt = __popc(nib[u]), inc = wave_inclusive_scan(cnt);
            loc[u] = wtotal + inc - cnt;
            wtotal += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        if (lane == 0) tot[par][wave] = wtotal;
        hj_barrier_lds();
        const uint4 t4 = *reinterpret_cast<const uint4 *>(tot[par]);
        const uint32_t before = hj_uniform((wave > 0 ? t4.x : 0u) + (wave > 1 ? t4.y : 0u) + (wave > 2 ? t4.z : 0u));
        const u64 wbase = run + before;
        run += hj_uniform(t4.x + t4.y + t4.z + t4.w);
        if constexpr (STAGED) {
            constexpr int OUTS = NCOLS + (ROWS ? 1 : 0);
#pragma unroll
            for (int c = 0; c < OUTS; ++c) {
#pragma unroll
                for (int u = 0; u < VEC; ++u) {
                    uint32_t at = loc[u];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((nib[u] >> j) & 1u) {
                            uint32_t x;
                            if (c < NCOLS) x = compact_elem(kk[c < NCOLS ? c : 0][u], j);
                            else x = (uint32_t)(((v0 + (u64)u * 64) << 2) + j);
                            stage[wave][at++] = x;
                        }
                }
                compact_wave_sync();
                uint32_t *out = c < NCOLS ? a.out[c < NCOLS ? c : 0] : a.rows_out;
                for (uint32_t e = lane; e < wtotal; e += 64) {
                    const uint32_t x = stage[wave][e];
                    if (wbase + e < a.capacity) hj_store(out + wbase + e, x);
                }
                compact_wave_sync();
            }
        } else {
#pragma unroll
            for (int u = 0; u < VEC; ++u) {
                u64 o = wbase + loc[u];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((nib[u] >> j) & 1u) {
                        if (o < a.capacity) {
#pragma unroll
                            for (int c = 0; c < NCOLS; ++c) hj_store(a.out[c] + o, compact_elem(kk[c][u], j));
                            if constexpr (ROWS) hj_store(a.rows_out + o, (uint32_t)(((v0 + (u64)u * 64) << 2) + j));
                        }
                        ++o;
                    }
            }
        }
    }
}

// how the survivors reach memory (see compact_kernel; DESIGN.md section 5 records both)
#ifndef HJ_COMPACT_STAGED
#define HJ_COMPACT_STAGED 1
#endif

template <int NCOLS, bool ROWS>
static void compact_launch(const CompactArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL((compact_kernel<NCOLS, ROWS, HJ_COMPACT_STAGED != 0>), dim3(a.lay.ranges), dim3(hj_compact::BLOCK), 0, stream, a);
}

int hj_launch_compact_count(const uint32_t *select_bits, const hj_compact::Layout &lay, u64 *counts, hipStream_t stream)
{
    hipLaunchKernelGGL(compact_count_kernel, dim3(lay.ranges), dim3(hj_compact::BLOCK), 0, stream, select_bits, lay, counts);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_compact_total(const u64 *counts, uint32_t ranges, u64 *d_count, hipStream_t stream)
{
    hipLaunchKernelGGL(compact_total_kernel, dim3(1), dim3(256), 0, stream, counts, ranges, d_count);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// one launch: ncols <= HJ_COMPACT_LAUNCH_COLS columns (a.in / a.out [0 .. ncols)), the row numbers when a.rows_out is set; never neither
int hj_launch_compact(const CompactArgs &a, uint32_t ncols, hipStream_t stream)
{
    const bool rows = a.rows_out != nullptr;
    if (ncols > HJ_COMPACT_LAUNCH_COLS || (ncols == 0 && !rows)) return HJGPU_EINVAL;
    hj_with_bool(rows, [&](auto r) {
        constexpr bool R = decltype(r)::value;
        switch (ncols) {
        case 0: if constexpr (R) compact_launch<0, true>(a, stream); break;
        case 1: compact_launch<1, R>(a, stream); break;
        case 2: compact_launch<2, R>(a, stream); break;
        case 3: compact_launch<3, R>(a, stream); break;
        default: compact_launch<4, R>(a, stream); break;
        }
    });
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// ---- grouped aggregation (hjgpu_group_sum; DESIGN.md section 5 "Grouped aggregation") -------------------------------------------------
// GROUP BY (key 0 [, key 1]) COUNT(*), SUM(measure 0 ... nvals - 1) over the rows a bitmap selects.  The tables are group_layout.hpp's: a
// slot is the tuple in one 64-bit word, a count and four sums; a hashed slot is occupied when that word is not 0, the tuple 0 has the
// slot behind the hashed ones.  Insert-or-find is ONE 64-bit compare-and-swap of the tuple word (ds_cmpst_rtn_b64 in LDS,
// global_atomic_cmpswap_x2 in the merge table): a slot is never half written, so nobody waits - a claim-then-publish state word would make
// the lanes of a wave wait for one another.  Counts and sums are 64-bit atomic adds.  The kernel has no global store at all.
constexpr u64 GROUP_NO_SLOT = 1ull << 62;               // a row whose tuple found no slot in the merge table (the overflow word is raised)
constexpr u64 GROUP_IN_LDS = 1ull << 63;                // a location in the workgroup's table: this bit and the slot's index

// The slot of tuple t (hash h) in the workgroup's table, GROUP_NO_SLOT when the row has to go to the merge table: after LDS_PROBES slots
// that hold other tuples, or at an empty slot once the table has claimed LDS_GROUPS hashed slots (`used` is a ticket: taken before the
// claim and handed back when the claim fails, so the table never holds more).
__device__ __forceinline__ u64 group_lds_slot(hj_group::Slot *tab, uint32_t *used, u64 t, u64 h)
{
    using namespace hj_group;
    if (t == 0) return GROUP_IN_LDS | LDS_SLOTS;
    uint32_t s = lds_home(h);
#pragma unroll 1
    for (uint32_t p = 0; p < LDS_PROBES; ++p) {
        u64 cur = __hip_atomic_load(&tab[s].tuple, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) {
            if (__hip_atomic_load(used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= LDS_GROUPS) return GROUP_NO_SLOT;   // (a broadcast read: no ticket traffic once the table is full)
            if (atomicAdd(used, 1u) >= LDS_GROUPS) { atomicSub(used, 1u); return GROUP_NO_SLOT; }
            cur = atomicCAS(&tab[s].tuple, 0ull, t);                    // ds_cmpst_rtn_b64
            if (cur == 0) return GROUP_IN_LDS | s;
            atomicSub(used, 1u);
        }
        if (cur == t) return GROUP_IN_LDS | s;
        s = (s + 1) & (LDS_SLOTS - 1);
    }
    return GROUP_NO_SLOT;
}

// The slot of tuple t in the merge table: linear probing bounded by the slot count.  A tuple that finds the table full raises the
// overflow word; whoever sees it raised gives up at once - the call has overflowed, what it leaves below capacity is unspecified, and
// the full table is the lower bound of the group count - so an overflowing call does not walk a full table once per row.
__device__ __forceinline__ u64 group_merge_slot(const GroupArgs &a, u64 t, u64 h)
{
    if (t == 0) return a.merge_mask + 1;
    if (__hip_atomic_load(a.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return GROUP_NO_SLOT;
    u64 s = h & a.merge_mask;
    for (u64 p = 0; p <= a.merge_mask; ++p) {
        u64 cur = __hip_atomic_load(&a.merge[s].tuple, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) cur = atomicCAS(&a.merge[s].tuple, 0ull, t);
        if (cur == 0 || cur == t) return s;
        s = (s + 1) & a.merge_mask;
    }
    atomicOr(a.overflow, 1u);
    return GROUP_NO_SLOT;
}

// combines x into word `word` (0: the count, 1 + c: sum or aggregate c) of the slot at `loc` of either table layout - group_layout.hpp's or
// wide_group_layout.hpp's slots, which both end in the count and four words: added, or the unsigned maximum for an extreme
template <class Slot>
__device__ __forceinline__ void group_combine(Slot *tab, Slot *merge, u64 loc, uint32_t word, bool extreme, u64 x)
{
    if (loc & GROUP_IN_LDS) {
        u64 *p = &tab[(uint32_t)loc].count + word;
        if (extreme) __hip_atomic_fetch_max(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);                     // ds_max_u64
        else __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);                             // ds_add_u64
    } else if (loc != GROUP_NO_SLOT) {
        u64 *p = &merge[loc].count + word;
        if (extreme) __hip_atomic_fetch_max(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                         // global_atomic_umax_x2
        else atomicAdd(p, x);                                                                                           // global_atomic_add_x2
    }
}

// One persistent grid.  An iteration is BATCH wave trips of hj_lookup.hpp's layout (lane L owns rows 4 L ... 4 L + 3 of a trip): the mask
// words first, then key column 0 (lookup_fetch), then key column 1 and, one after the other, the measure columns for the lanes that have a
// selected row - a group of 8 lanes whose mask word is 0 loads nothing from any column; everything non-temporal; the last, partial vector
// of a column is loaded whole and masked, as lookup_fetch does.  A lane folds those of its four rows that carry the same tuple (cls: for
// every row the set of rows it leads, a nibble each), finds the leaders' slots - the workgroup's table, else the merge table - and adds the
// counts; then, per measure column (nvals is a uniform run-time bound), it loads the column and adds each leader's sum to its slot.  At the
// end the workgroup adds its occupied slots to the merge table.  No workgroup waits for another.
template <int NKEYS, bool SEL>
__global__ __launch_bounds__(hj_group::BLOCK) void group_sum_kernel(GroupArgs a)
{
    using namespace hj_group;
    constexpr int BATCH = 2, ROWS = 4 * BATCH;
    __shared__ Slot tab[LDS_SLOTS + 1];
    __shared__ uint32_t used;
    const uint32_t tid = threadIdx.x;
    {
        u64 *raw = reinterpret_cast<u64 *>(tab);
        for (uint32_t i = tid; i < (LDS_SLOTS + 1) * (uint32_t)(sizeof(Slot) / 8); i += BLOCK) raw[i] = 0;
        if (tid == 0) used = 0;
    }
    __syncthreads();
    const uint4 *k4 = reinterpret_cast<const uint4 *>(a.keys[0]);
    const uint4 *k4b = reinterpret_cast<const uint4 *>(a.keys[NKEYS - 1]);
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    const uint32_t nvals = a.nvals;
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t nib[BATCH];
        uint4 k0[BATCH], k1[BATCH];
        lookup_fetch<SEL, BATCH, true>(a.select_bits, k4, v0, stride, n, nib, k0);
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            k1[u] = make_uint4(0, 0, 0, 0);
            if constexpr (NKEYS == 2) { if (nib[u]) k1[u] = hj_load_nt(k4b + v0 + (u64)u * stride + hj_lane()); }
        }
        // the fold: row q = 4 u + j of the lane leads the rows of its trip that carry its tuple and that no earlier row leads
        u64 t[ROWS], loc[ROWS];
        uint32_t cls = 0, lead = 0;                     // cls: a nibble per row, the rows (of its trip) it leads; lead: the rows that lead any
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            t[4 * u] = tuple_of(k0[u].x, k1[u].x); t[4 * u + 1] = tuple_of(k0[u].y, k1[u].y);
            t[4 * u + 2] = tuple_of(k0[u].z, k1[u].z); t[4 * u + 3] = tuple_of(k0[u].w, k1[u].w);
            uint32_t left = nib[u];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                loc[4 * u + j] = GROUP_NO_SLOT;
                uint32_t m = 0;
#pragma unroll
                for (int i = j; i < 4; ++i) if (((left >> i) & 1u) && t[4 * u + i] == t[4 * u + j]) m |= 1u << i;
                if (!((left >> j) & 1u)) m = 0;
                left &= ~m;
                cls |= m << (4 * (4 * u + j));
                lead |= (m ? 1u : 0u) << (4 * u + j);
            }
        }
        // the leaders' slots and counts: one copy of the probe code, whichever row it serves
        for (uint32_t work = lead; work; work &= work - 1) {
            const uint32_t q = __ffs(work) - 1;
            u64 tu[4] = {t[0], t[1], t[2], t[3]};       // the trip's, then the row's
#pragma unroll
            for (int u = 1; u < BATCH; ++u)
                if ((int)(q >> 2) == u) { tu[0] = t[4 * u]; tu[1] = t[4 * u + 1]; tu[2] = t[4 * u + 2]; tu[3] = t[4 * u + 3]; }
            const uint32_t qj = q & 3u;
            const u64 tq = qj == 0 ? tu[0] : qj == 1 ? tu[1] : qj == 2 ? tu[2] : tu[3];
            const u64 h = mix(tq);
            u64 at = group_lds_slot(tab, &used, tq, h);
            if (at == GROUP_NO_SLOT) at = group_merge_slot(a, tq, h);
            group_combine(tab, a.merge, at, 0, false, (u64)__popc((cls >> (4 * q)) & 15u));
#pragma unroll
            for (int r = 0; r < ROWS; ++r) loc[r] = q == r ? at : loc[r];
        }
        for (uint32_t c = 0; c < nvals; ++c) {
            const uint4 *x4 = reinterpret_cast<const uint4 *>(a.vals[c]);
            uint4 x[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                x[u] = make_uint4(0, 0, 0, 0);
                if (nib[u]) x[u] = hj_load_nt(x4 + v0 + (u64)u * stride + hj_lane());
            }
            for (uint32_t work = lead; work; work &= work - 1) {
                const uint32_t q = __ffs(work) - 1, m = (cls >> (4 * q)) & 15u;
                uint4 xq = x[0];
#pragma unroll
                for (int u = 1; u < BATCH; ++u) if ((int)(q >> 2) == u) xq = x[u];
                u64 at = loc[0];
#pragma unroll
                for (int r = 1; r < ROWS; ++r) at = q == r ? loc[r] : at;
                const u64 sum = (u64)((m & 1u) ? xq.x : 0u) + ((m & 2u) ? xq.y : 0u) + ((m & 4u) ? xq.z : 0u) + ((m & 8u) ? xq.w : 0u);
                group_combine(tab, a.merge, at, 1 + c, false, sum);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i <= LDS_SLOTS; i += BLOCK) {
        const u64 t = tab[i].tuple, cnt = tab[i].count;
        if (i < LDS_SLOTS ? t != 0 : cnt != 0) {
            const u64 at = group_merge_slot(a, t, mix(t));
            if (at != GROUP_NO_SLOT) {
                atomicAdd(&a.merge[at].count, cnt);
                for (uint32_t c = 0; c < nvals; ++c) atomicAdd(&a.merge[at].sums[c], tab[i].sums[c]);
            }
        }
    }
}

// ---- aggregate functions (hjgpu_group_agg; DESIGN.md section 5 "Aggregate functions") ---------------------------------------------------
// GROUP BY (nothing | key 0 [, key 1]) COUNT(*) and up to four of SUM(a), SUM(a * b), MIN(a), MAX(a) over the rows a bitmap selects.  The
// grouped road is group_sum_kernel's body with two differences: what a row contributes to an aggregate's word of its slot, and how words
// are combined - agg_layout.hpp's term() and combine(): a sum is added, an extreme is an unsigned maximum of a transformed value whose
// neutral word is the tables' initial 0 (ds_max_u64 in LDS, global_atomic_umax_x2 in the merge table).  fn and flags are uniform run-time
// values per aggregate: every branch on them is a scalar branch.  The tables, insert-or-find, the fold, the spill rule and the flush are
// group_sum_kernel's own (group_lds_slot, group_merge_slot, group_combine).

// the terms of the rows of nibble m of one vector, combined: a row outside m contributes the neutral 0.  Straight-line code: the terms of
// all four rows are computed and chosen by the nibble's bits
template <int KIND>
__device__ __forceinline__ u64 agg_fold(const hj_agg::Norm &p, uint32_t m, const uint4 &x, const uint4 &y)
{
    using namespace hj_agg;
    u64 acc = (m & 1u) ? term<KIND>(p, x.x, y.x) : 0ull;
    acc = combine<KIND>(acc, (m & 2u) ? term<KIND>(p, x.y, y.y) : 0ull);
    acc = combine<KIND>(acc, (m & 4u) ? term<KIND>(p, x.z, y.z) : 0ull);
    return combine<KIND>(acc, (m & 8u) ? term<KIND>(p, x.w, y.w) : 0ull);
}

// agg_fold under the aggregate's own kind: fn is uniform, so this is a scalar branch to one of three straight-line bodies
__device__ __forceinline__ u64 agg_fold_of(uint32_t fn, const hj_agg::Norm &p, uint32_t m, const uint4 &x, const uint4 &y)
{
    using namespace hj_agg;
    if (fn == SUM) return agg_fold<KIND_VALUE>(p, m, x, y);
    if (fn == SUM_MUL) return agg_fold<KIND_PRODUCT>(p, m, x, y);
    return agg_fold<KIND_EXTREME>(p, m, x, y);
}

// The scalar road's body for one aggregate of one kind: the vectors of a - and of b, KIND_PRODUCT only - of the lane's trips (v: the first
// trip's vector) for the lanes whose nibble is not 0 (nib != 0 only where the vector starts below n), then their folded terms, combined.
// The loads sit inside the body, so the three kinds are three real branches and a row costs the arithmetic of its own kind alone.
template <int KIND, int BATCH>
__device__ __forceinline__ u64 agg_scalar_part(const hj_agg::Norm &p, const uint32_t (&nib)[BATCH], const uint4 *x4, const uint4 *y4, u64 v, u64 stride)
{
    uint4 x[BATCH], y[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
        x[u] = make_uint4(0, 0, 0, 0);
        if (nib[u]) x[u] = hj_load_nt(x4 + v + (u64)u * stride);
    }
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
        y[u] = make_uint4(0, 0, 0, 0);
        if constexpr (KIND == hj_agg::KIND_PRODUCT) { if (nib[u]) y[u] = hj_load_nt(y4 + v + (u64)u * stride); }
    }
    u64 part = 0;
#pragma unroll
    for (int u = 0; u < BATCH; ++u) part = hj_agg::combine<KIND>(part, agg_fold<KIND>(p, nib[u], x[u], y[u]));
    return part;
}

// group_sum_kernel's iteration up to the leaders' slots and counts; then, per aggregate (naggs is a uniform run-time bound), column a - and
// column b under SUM_MUL - loaded as the measure columns are: non-temporal, only by the lanes whose nibble is not 0, the last partial vector
// whole and masked by the nibble; each leader's folded term goes to its slot.  The flush combines the workgroup's occupied slots into the
// merge table, word by word under the word's own combine.  No global store; no workgroup waits for another.
template <int NKEYS, bool SEL>
__global__ __launch_bounds__(hj_group::BLOCK) void agg_group_kernel(AggArgs aa)
{
    using namespace hj_group;
    constexpr int BATCH = (int)hj_agg::GROUP_BATCH, ROWS = 4 * BATCH;
    const GroupArgs &a = aa.g;
    __shared__ Slot tab[LDS_SLOTS + 1];
    __shared__ uint32_t used;
    const uint32_t tid = threadIdx.x;
    {
        u64 *raw = reinterpret_cast<u64 *>(tab);
        for (uint32_t i = tid; i < (LDS_SLOTS + 1) * (uint32_t)(sizeof(Slot) / 8); i += BLOCK) raw[i] = 0;
        if (tid == 0) used = 0;
    }
    __syncthreads();
    const uint4 *k4 = reinterpret_cast<const uint4 *>(a.keys[0]);
    const uint4 *k4b = reinterpret_cast<const uint4 *>(a.keys[NKEYS - 1]);
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    const uint32_t naggs = a.nvals;
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t nib[BATCH];
        uint4 k0[BATCH], k1[BATCH];
        lookup_fetch<SEL, BATCH, true>(a.select_bits, k4, v0, stride, n, nib, k0);
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            k1[u] = make_uint4(0, 0, 0, 0);
            if constexpr (NKEYS == 2) { if (nib[u]) k1[u] = hj_load_nt(k4b + v0 + (u64)u * stride + hj_lane()); }
        }
        // the fold: row q = 4 u + j of the lane leads the rows of its trip that carry its tuple and that no earlier row leads
        u64 t[ROWS], loc[ROWS];
        uint32_t cls = 0, lead = 0;                     // cls: a nibble per row, the rows (of its trip) it leads; lead: the rows that lead any
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            t[4 * u] = tuple_of(k0[u].x, k1[u].x); t[4 * u + 1] = tuple_of(k0[u].y, k1[u].y);
            t[4 * u + 2] = tuple_of(k0[u].z, k1[u].z); t[4 * u + 3] = tuple_of(k0[u].w, k1[u].w);
            uint32_t left = nib[u];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                loc[4 * u + j] = GROUP_NO_SLOT;
                uint32_t m = 0;
#pragma unroll
                for (int i = j; i < 4; ++i) if (((left >> i) & 1u) && t[4 * u + i] == t[4 * u + j]) m |= 1u << i;
                if (!((left >> j) & 1u)) m = 0;
                left &= ~m;
                cls |= m << (4 * (4 * u + j));
                lead |= (m ? 1u : 0u) << (4 * u + j);
            }
        }
        // the leaders' slots and counts: one copy of the probe code, whichever row it serves
        for (uint32_t work = lead; work; work &= work - 1) {
            const uint32_t q = __ffs(work) - 1;
            u64 tu[4] = {t[0], t[1], t[2], t[3]};       // the trip's, then the row's
#pragma unroll
            for (int u = 1; u < BATCH; ++u)
                if ((int)(q >> 2) == u) { tu[0] = t[4 * u]; tu[1] = t[4 * u + 1]; tu[2] = t[4 * u + 2]; tu[3] = t[4 * u + 3]; }
            const uint32_t qj = q & 3u;
            const u64 tq = qj == 0 ? tu[0] : qj == 1 ? tu[1] : qj == 2 ? tu[2] : tu[3];
            const u64 h = mix(tq);
            u64 at = group_lds_slot(tab, &used, tq, h);
            if (at == GROUP_NO_SLOT) at = group_merge_slot(a, tq, h);
            group_combine(tab, a.merge, at, 0, false, (u64)__popc((cls >> (4 * q)) & 15u));
#pragma unroll
            for (int r = 0; r < ROWS; ++r) loc[r] = q == r ? at : loc[r];
        }
        for (uint32_t c = 0; c < naggs; ++c) {
            const uint32_t fn = aa.fn[c];
            const hj_agg::Norm norm = hj_agg::normalise(fn, aa.flags[c]);
            const uint4 *x4 = reinterpret_cast<const uint4 *>(a.vals[c]);
            const uint4 *y4 = reinterpret_cast<const uint4 *>(aa.b[c]);
            uint4 x[BATCH], y[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                x[u] = make_uint4(0, 0, 0, 0);
                if (nib[u]) x[u] = hj_load_nt(x4 + v0 + (u64)u * stride + hj_lane());
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                y[u] = make_uint4(0, 0, 0, 0);
                if (fn == hj_agg::SUM_MUL && nib[u]) y[u] = hj_load_nt(y4 + v0 + (u64)u * stride + hj_lane());
            }
            const bool extreme = hj_agg::is_extreme(fn);
            for (uint32_t work = lead; work; work &= work - 1) {
                const uint32_t q = __ffs(work) - 1, m = (cls >> (4 * q)) & 15u;
                uint4 xq = x[0], yq = y[0];
#pragma unroll
                for (int u = 1; u < BATCH; ++u) if ((int)(q >> 2) == u) { xq = x[u]; yq = y[u]; }
                u64 at = loc[0];
#pragma unroll
                for (int r = 1; r < ROWS; ++r) at = q == r ? loc[r] : at;
                group_combine(tab, a.merge, at, 1 + c, extreme, agg_fold_of(fn, norm, m, xq, yq));
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i <= LDS_SLOTS; i += BLOCK) {
        const u64 t = tab[i].tuple, cnt = tab[i].count;
        if (i < LDS_SLOTS ? t != 0 : cnt != 0) {
            const u64 at = group_merge_slot(a, t, mix(t));
            if (at != GROUP_NO_SLOT) {
                atomicAdd(&a.merge[at].count, cnt);
                for (uint32_t c = 0; c < naggs; ++c) {
                    if (hj_agg::is_extreme(aa.fn[c])) __hip_atomic_fetch_max(&a.merge[at].sums[c], tab[i].sums[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else atomicAdd(&a.merge[at].sums[c], tab[i].sums[c]);
                }
            }
        }
    }
}

__device__ __forceinline__ u64 agg_wave_reduce(bool extreme, u64 x)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 y = __shfl_down(x, d, 64);
        x = extreme ? (y > x ? y : x) : x + y;
    }
    return x;   // valid in lane 0
}

// The scalar road (nkeys == 0): no table.  One persistent grid of agg_layout.hpp's scalar geometry; an iteration is BATCH wave trips of
// hj_lookup.hpp's layout: the mask words first (SEL; lookup_fetch's nibble, cut at n), then, per aggregate, column a - and column b under
// SUM_MUL - for the lanes whose nibble is not 0: a group of 8 lanes whose mask word is 0 loads nothing; everything non-temporal; the last,
// partial vector of a column is loaded whole and masked by the nibble.  A lane keeps the count and the aggregates' words in registers over
// its whole loop; at the end a wave combines them across its lanes, the workgroup's waves through LDS - the kernel's only LDS, behind the
// loop - and one lane combines them into the merge table's slot of tuple 0 (a.g.merge[a.g.merge_mask + 1]), which the emit kernel turns
// into J = 1 when its count is not 0.  No global store; no workgroup waits for another.
template <bool SEL>
__global__ __launch_bounds__(hj_agg::SCALAR_BLOCK) void agg_scalar_kernel(AggArgs aa)
{
    using namespace hj_agg;
    constexpr int BATCH = (int)SCALAR_BATCH, NW = SCALAR_BLOCK / 64;
    __shared__ u64 red[NW][1 + MAX_AGGS];
    const GroupArgs &a = aa.g;
    const uint32_t tid = threadIdx.x;
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * SCALAR_BLOCK;
    const uint32_t naggs = a.nvals;
    u64 count = 0, acc[MAX_AGGS] = {0, 0, 0, 0};
    for (u64 v0 = (u64)blockIdx.x * SCALAR_BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t nib[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const u64 v = v0 + (u64)u * stride + hj_lane(), g = v << 2;
            const uint32_t rows = g + 4 <= n ? 15u : g < n ? (1u << (uint32_t)(n - g)) - 1u : 0u;
            nib[u] = rows;
            if constexpr (SEL) {
                uint32_t w = 0;
                if (v < nvec) w = hj_load_nt(a.select_bits + (v >> 3));     // (v < nvec: row 4 v < n, and word v / 8 starts at or before it)
                nib[u] = (w >> ((tid & 7u) * 4)) & rows;
            }
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) count += __popc(nib[u]);
        // (one copy of the body for whichever aggregate it serves, as the measure loop of group_sum_kernel: unrolled copies would keep
        // every aggregate's vectors in registers at once and halve the waves per SIMD)
#pragma unroll 1
        for (uint32_t c = 0; c < naggs; ++c) {
            const uint32_t fn = aa.fn[c];
            const Norm norm = normalise(fn, aa.flags[c]);
            const uint4 *x4 = reinterpret_cast<const uint4 *>(a.vals[c]);
            const uint4 *y4 = reinterpret_cast<const uint4 *>(aa.b[c]);
            const u64 v = v0 + hj_lane();
            u64 part;
            if (fn == SUM) part = agg_scalar_part<KIND_VALUE, BATCH>(norm, nib, x4, y4, v, stride);
            else if (fn == SUM_MUL) part = agg_scalar_part<KIND_PRODUCT, BATCH>(norm, nib, x4, y4, v, stride);
            else part = agg_scalar_part<KIND_EXTREME, BATCH>(norm, nib, x4, y4, v, stride);
#pragma unroll
            for (uint32_t k = 0; k < MAX_AGGS; ++k) acc[k] = k == c ? combine(fn, acc[k], part) : acc[k];   // (c is uniform: a scalar compare, no indexed register)
        }
    }
    count = wave_reduce_sum(count);
#pragma unroll
    for (uint32_t c = 0; c < MAX_AGGS; ++c)
        if (c < naggs) acc[c] = agg_wave_reduce(is_extreme(aa.fn[c]), acc[c]);
    if (hj_lane() == 0) {
        red[tid >> 6][0] = count;
#pragma unroll
        for (uint32_t c = 0; c < MAX_AGGS; ++c) red[tid >> 6][1 + c] = acc[c];
    }
    __syncthreads();
    if (tid == 0) {
        hj_group::Slot *slot = a.merge + (a.merge_mask + 1);
        u64 rows = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) rows += red[w][0];
        if (rows) {                                                     // (no selected row: nothing to combine, and the count stays 0)
            atomicAdd(&slot->count, rows);
#pragma unroll
            for (uint32_t c = 0; c < MAX_AGGS; ++c) {
                if (c >= naggs) break;
                const uint32_t fn = aa.fn[c];
                u64 x = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) x = combine(fn, x, red[w][1 + c]);
                if (is_extreme(fn)) __hip_atomic_fetch_max(&slot->sums[c], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else atomicAdd(&slot->sums[c], x);
            }
        }
    }
}

// ---- wide keys (hjgpu_group_by with three and four key columns; DESIGN.md section 5 "Wide keys") ---------------------------------------
// GROUP BY (key 0, key 1, key 2 [, key 3]) COUNT(*) and hjgpu_group_agg's aggregates.  A tuple no longer fits the one 64-bit word that
// group_lds_slot / group_merge_slot compare and swap, and there is no 128-bit compare-and-swap: the tables are wide_group_layout.hpp's -
// a slot has a 64-bit word per key, key | 1 << 32, never 0 - and insert-or-find is that header's find_slot: word by word, a 64-bit
// compare-and-swap 0 -> own word wherever a word is still 0 (ds_cmpst_rtn_b64 in LDS, global_atomic_cmpswap_x2 in the merge table), on to
// the next slot at the first word that is another tuple's.  Nobody waits and no slot stays half filled.  The words of the aggregates and
// their combines are agg_group_kernel's (group_combine).

// the two memories of find_slot: relaxed atomics of workgroup scope in LDS - `used` is group_lds_slot's ticket, taken before a slot's word
// 0 is written and handed back when that write lost, so the table never holds more than LDS_GROUPS tuples - and of agent scope in the
// merge table, where every slot may be claimed
struct WideLdsMemory {
    uint32_t *used;
    __device__ __forceinline__ u64 load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ u64 cas(u64 *p, u64 word) { return atomicCAS(p, 0ull, word); }                          // ds_cmpst_rtn_b64
    __device__ __forceinline__ bool claim()
    {
        if (__hip_atomic_load(used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= hj_wide::LDS_GROUPS) return false;  // (a broadcast read: no ticket traffic once the table is full)
        if (atomicAdd(used, 1u) >= hj_wide::LDS_GROUPS) { atomicSub(used, 1u); return false; }
        return true;
    }
    __device__ __forceinline__ void unclaim() { atomicSub(used, 1u); }
};
struct WideGlobalMemory {
    __device__ __forceinline__ u64 load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ u64 cas(u64 *p, u64 word) { return atomicCAS(p, 0ull, word); }                          // global_atomic_cmpswap_x2
    __device__ __forceinline__ bool claim() { return true; }
    __device__ __forceinline__ void unclaim() {}
};

// The slot of the tuple with key words w (hash h) in the merge table: the walk bounded by the slot count; group_merge_slot's overflow rule -
// a tuple that finds the table full raises the overflow word, whoever sees it raised gives up at once
template <int NKEYS>
__device__ __forceinline__ u64 wide_merge_slot(const decltype(WideArgs::g) &a, const u64 (&w)[hj_wide::MAX_KEYS], u64 h)
{
    if (__hip_atomic_load(a.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return GROUP_NO_SLOT;
    WideGlobalMemory mem;
    const u64 s = hj_wide::find_slot<(uint32_t)NKEYS>(mem, a.merge, a.merge_mask, h, a.merge_mask + 1, w);
    if (s == hj_wide::NO_SLOT) atomicOr(a.overflow, 1u);
    return s;
}

// agg_group_kernel's iteration with NKEYS key columns: the mask words and key column 0 (lookup_fetch), then the further key columns and, per
// aggregate, column a - and b under SUM_MUL - for the lanes whose nibble is not 0; everything non-temporal; the last, partial vector of a
// column is loaded whole and masked by the nibble.  A lane folds those of its four rows that carry the same tuple onto leaders, the leaders
// find their slots - the workgroup's table, else the merge table - by find_slot, and each leader's folded term goes to its slot.  The walk
// over the leaders stays in the kernel's body (a helper that took the trips' vectors made the compiler index them in memory).  The flush
// combines the workgroup's occupied slots into the merge table, word by word.  No global store; no workgroup waits for another.
template <int NKEYS, bool SEL>
__global__ __launch_bounds__(hj_wide::BLOCK) void wide_group_kernel(WideArgs aa)
{
    using namespace hj_wide;
    const auto &a = aa.g;
    static_assert(NKEYS >= (int)MIN_KEYS && NKEYS <= (int)MAX_KEYS, "three or four key columns");
    static_assert(NO_SLOT == GROUP_NO_SLOT, "one word for \"no slot\" in the walk and in the locations");
    constexpr int ROWS = 4 * (int)BATCH, NB = (int)BATCH;
    __shared__ Slot tab[LDS_SLOTS];
    __shared__ uint32_t used;
    const uint32_t tid = threadIdx.x;
    {
        u64 *raw = reinterpret_cast<u64 *>(tab);
        for (uint32_t i = tid; i < LDS_SLOTS * (uint32_t)(sizeof(Slot) / 8); i += BLOCK) raw[i] = 0;
        if (tid == 0) used = 0;
    }
    __syncthreads();
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    const uint32_t naggs = a.nvals;
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * NB) {
        uint32_t nib[NB];
        uint32_t key[NKEYS][ROWS];                      // key column c of row 4 u + j of the lane
        {
            uint4 k0[NB];
            lookup_fetch<SEL, NB, true>(a.select_bits, reinterpret_cast<const uint4 *>(a.keys[0]), v0, stride, n, nib, k0);
#pragma unroll
            for (int u = 0; u < NB; ++u) { key[0][4 * u] = k0[u].x; key[0][4 * u + 1] = k0[u].y; key[0][4 * u + 2] = k0[u].z; key[0][4 * u + 3] = k0[u].w; }
        }
#pragma unroll
        for (int c = 1; c < NKEYS; ++c) {
            const uint4 *k4 = reinterpret_cast<const uint4 *>(a.keys[c]);
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                uint4 kc = make_uint4(0, 0, 0, 0);
                if (nib[u]) kc = hj_load_nt(k4 + v0 + (u64)u * stride + hj_lane());
                key[c][4 * u] = kc.x; key[c][4 * u + 1] = kc.y; key[c][4 * u + 2] = kc.z; key[c][4 * u + 3] = kc.w;
            }
        }
        // the fold: row q = 4 u + j of the lane leads the rows of its trip that carry its tuple and that no earlier row leads
        u64 loc[ROWS];
        uint32_t cls = 0, lead = 0;                     // cls: a nibble per row, the rows (of its trip) it leads; lead: the rows that lead any
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            uint32_t left = nib[u];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                loc[4 * u + j] = GROUP_NO_SLOT;
                uint32_t m = 0;
#pragma unroll
                for (int i = j; i < 4; ++i) {
                    bool same = true;
#pragma unroll
                    for (int c = 0; c < NKEYS; ++c) same = same && key[c][4 * u + i] == key[c][4 * u + j];
                    if (((left >> i) & 1u) && same) m |= 1u << i;
                }
                if (!((left >> j) & 1u)) m = 0;
                left &= ~m;
                cls |= m << (4 * (4 * u + j));
                lead |= (m ? 1u : 0u) << (4 * u + j);
            }
        }
        // the leaders' slots and counts: one copy of the walk, whichever row it serves
        for (uint32_t work = lead; work; work &= work - 1) {
            const uint32_t q = __ffs(work) - 1;
            u64 w[MAX_KEYS] = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < NKEYS; ++c) {
                uint32_t kq = key[c][0];
#pragma unroll
                for (int r = 1; r < ROWS; ++r) kq = q == r ? key[c][r] : kq;
                w[c] = key_word(kq);
            }
            const u64 h = hash(w);
            WideLdsMemory lds{&used};
            u64 at = find_slot<(uint32_t)NKEYS>(lds, tab, LDS_SLOTS - 1, lds_home(h), LDS_PROBES, w);
            if (at != NO_SLOT) at |= GROUP_IN_LDS;
            else at = wide_merge_slot<NKEYS>(a, w, h);
            group_combine(tab, a.merge, at, 0, false, (u64)__popc((cls >> (4 * q)) & 15u));
#pragma unroll
            for (int r = 0; r < ROWS; ++r) loc[r] = q == r ? at : loc[r];
        }
        for (uint32_t c = 0; c < naggs; ++c) {
            const uint32_t fn = aa.fn[c];
            const hj_agg::Norm norm = hj_agg::normalise(fn, aa.flags[c]);
            const uint4 *x4 = reinterpret_cast<const uint4 *>(a.vals[c]);
            const uint4 *y4 = reinterpret_cast<const uint4 *>(aa.b[c]);
            uint4 x[NB], y[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                x[u] = make_uint4(0, 0, 0, 0);
                if (nib[u]) x[u] = hj_load_nt(x4 + v0 + (u64)u * stride + hj_lane());
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                y[u] = make_uint4(0, 0, 0, 0);
                if (fn == hj_agg::SUM_MUL && nib[u]) y[u] = hj_load_nt(y4 + v0 + (u64)u * stride + hj_lane());
            }
            const bool extreme = hj_agg::is_extreme(fn);
            for (uint32_t work = lead; work; work &= work - 1) {
                const uint32_t q = __ffs(work) - 1, m = (cls >> (4 * q)) & 15u;
                uint4 xq = x[0], yq = y[0];
#pragma unroll
                for (int u = 1; u < NB; ++u) if ((int)(q >> 2) == u) { xq = x[u]; yq = y[u]; }
                u64 at = loc[0];
#pragma unroll
                for (int r = 1; r < ROWS; ++r) at = q == r ? loc[r] : at;
                group_combine(tab, a.merge, at, 1 + c, extreme, agg_fold_of(fn, norm, m, xq, yq));
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < LDS_SLOTS; i += BLOCK) {
        if (tab[i].key[0] == 0) continue;
        u64 w[MAX_KEYS] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < NKEYS; ++c) w[c] = tab[i].key[c];
        const u64 at = wide_merge_slot<NKEYS>(a, w, hash(w));
        if (at != GROUP_NO_SLOT) {
            atomicAdd(&a.merge[at].count, tab[i].count);
            for (uint32_t c = 0; c < naggs; ++c) {
                if (hj_agg::is_extreme(aa.fn[c])) __hip_atomic_fetch_max(&a.merge[at].aggs[c], tab[i].aggs[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else atomicAdd(&a.merge[at].aggs[c], tab[i].aggs[c]);
            }
        }
    }
}

// ---- the emit of the three grouped operators --------------------------------------------------------------------------------------------
// What the one emit body has to know of a merge table: which slots there are behind the `slots` hashed ones (EMIT_EXTRA), what a lane
// keeps of slot i (Seen), when that slot is occupied, and where its key column c and its count lie.
struct NarrowEmitTable {                                // group_layout.hpp: the tuple word; the slot of tuple 0 is merge[slots], occupied when its count is not 0
    using Slot = hj_group::Slot;
    static constexpr uint32_t MAX_KEYS = hj_group::MAX_KEYS;
    static constexpr u64 EMIT_EXTRA = 1;
    struct Seen { u64 t, count; };
    __device__ __forceinline__ static Seen see(const Slot *merge, u64 i, u64 slots)
    {
        Seen s{0, 0};
        if (i <= slots) { s.t = merge[i].tuple; s.count = merge[i].count; }
        return s;
    }
    __device__ __forceinline__ static bool occupied(const Seen &s, u64 i, u64 slots) { return i < slots ? s.t != 0 : i == slots && s.count != 0; }
    __device__ __forceinline__ static uint32_t key(const Seen &s, const Slot &, uint32_t c) { return (uint32_t)(c == 0 ? s.t : s.t >> 32); }
    __device__ __forceinline__ static u64 count(const Seen &s, const Slot &) { return s.count; }
};
struct WideEmitTable {                                  // wide_group_layout.hpp: occupied when key word 0 is not 0; key column c is the low half of key word c
    using Slot = hj_wide::Slot;
    static constexpr uint32_t MAX_KEYS = hj_wide::MAX_KEYS;
    static constexpr u64 EMIT_EXTRA = 0;
    struct Seen { u64 w0; };
    __device__ __forceinline__ static Seen see(const Slot *merge, u64 i, u64 slots) { return Seen{i < slots ? merge[i].key[0] : 0}; }
    __device__ __forceinline__ static bool occupied(const Seen &s, u64, u64) { return s.w0 != 0; }
    __device__ __forceinline__ static uint32_t key(const Seen &s, const Slot &slot, uint32_t c) { return hj_wide::key_of(c == 0 ? s.w0 : slot.key[c]); }
    __device__ __forceinline__ static u64 count(const Seen &, const Slot &slot) { return slot.count; }
};
static_assert(sizeof(hj_group::Slot) - offsetof(hj_group::Slot, count) == (1 + hj_agg::MAX_AGGS) * sizeof(u64) &&
              sizeof(hj_wide::Slot) - offsetof(hj_wide::Slot, count) == (1 + hj_agg::MAX_AGGS) * sizeof(u64), "either slot ends in its count and four words");


// The body of the three emit kernels.  The occupied slots of the merge table go to the dense outputs, a wave's through one atomic add to
// the cursor, which is the count word itself (0 before the launch): behind the launch it holds the number of occupied slots - the group
// count J, or, when the overflow word was raised, the full table: a lower bound of J that is greater than capacity (the table has at least
// 2 * capacity slots).  Rows at capacity and beyond are counted and not written.  RESULT: agg_layout.hpp's result() per aggregate column -
// the sums leave as they are, the extremes in the column's own values (kinds: their functions).  Every store is hj_store.
template <class Table, bool RESULT, class Args, class Kinds>
__device__ __forceinline__ void group_emit_body(const Args &a, const Kinds &kinds)
{
    const uint32_t lane = hj_lane();
    const u64 total = a.slots + Table::EMIT_EXTRA, stride = (u64)gridDim.x * 256;
    for (u64 i0 = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < total; i0 += stride) {
        const u64 i = i0 + lane;
        const typename Table::Seen seen = Table::see(a.merge, i, a.slots);
        const bool occ = Table::occupied(seen, i, a.slots);
        const u64 vote = __ballot(occ);
        if (vote == 0) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(a.d_ngroups, (u64)__popcll(vote));
        base = hj_uniform(base);
        const u64 j = base + __popcll(vote & ((1ull << lane) - 1ull));
        if (occ && j < a.capacity) {
#pragma unroll
            for (uint32_t c = 0; c < Table::MAX_KEYS; ++c)
                if (c < a.nkeys) hj_store(a.keys_out[c] + j, Table::key(seen, a.merge[i], c));
            if (a.counts_out) hj_store(a.counts_out + j, Table::count(seen, a.merge[i]));
#pragma unroll
            for (uint32_t c = 0; c < hj_agg::MAX_AGGS; ++c) {
                if (c >= a.nvals) continue;
                u64 word = (&a.merge[i].count)[1 + c];
                if constexpr (RESULT) word = hj_agg::result(kinds.fn[c], kinds.flags[c], word);
                hj_store(a.sums_out[c] + j, word);
            }
        }
    }
}

__global__ __launch_bounds__(256) void group_emit_kernel(GroupEmitArgs a) { group_emit_body<NarrowEmitTable, false>(a, a); }
__global__ __launch_bounds__(256) void agg_emit_kernel(AggEmitArgs a) { group_emit_body<NarrowEmitTable, true>(a.g, a); }
__global__ __launch_bounds__(256) void wide_emit_kernel(WideEmitArgs a) { group_emit_body<WideEmitTable, true>(a.g, a); }

// The aggregation launches' check and grid: `per_cu` workgroups of `block` lanes per compute unit, no more than the rows have wave trips for
// (launch(sel, grid): the kernel with or without a mask)
template <class Args, class Launch>
static int grouped_launch(const Args &a, uint32_t min_keys, uint32_t max_keys, uint32_t block, int cus, uint32_t per_cu, Launch launch)
{
    const auto &g = a.g;
    if (g.n == 0) return HJGPU_OK;
    if (g.nkeys < min_keys || g.nkeys > max_keys || g.nvals > hj_agg::MAX_AGGS || !g.merge || !g.overflow || (g.merge_mask & (g.merge_mask + 1)) || cus < 1) return HJGPU_EINVAL;
    uintptr_t all = (uintptr_t)g.select_bits;
    for (uint32_t c = 0; c < g.nkeys; ++c) { if (!g.keys[c]) return HJGPU_EINVAL; all |= (uintptr_t)g.keys[c]; }
    for (uint32_t c = 0; c < g.nvals; ++c) {
        if (a.fn[c] > hj_agg::MAX || (a.flags[c] & ~hj_agg::SIGNED) || !g.vals[c] || (a.fn[c] == hj_agg::SUM_MUL) != (a.b[c] != nullptr)) return HJGPU_EINVAL;
        all |= (uintptr_t)g.vals[c] | (uintptr_t)a.b[c];
    }
    if (all & 15) return HJGPU_EINVAL;
    const u64 nvec = (g.n + 3) >> 2, need = (nvec + block - 1) / block;
    const dim3 grid((uint32_t)std::min<u64>(need, (u64)cus * per_cu));
    hj_with_bool(g.select_bits != nullptr, [&](auto sel) { launch(sel, grid); });
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// the grouped roads: one workgroup per compute unit (its table takes most of the unit's LDS)
int hj_launch_group_sum(const AggArgs &a, int cus, hipStream_t stream)
{
    using namespace hj_group;
    if (a.g.nvals > MAX_VALS) return HJGPU_EINVAL;
    for (uint32_t c = 0; c < a.g.nvals; ++c) if (a.fn[c] != hj_agg::SUM || a.flags[c]) return HJGPU_EINVAL;  // (the kernels read no function)
    return grouped_launch(a, 1, MAX_KEYS, BLOCK, cus, 1, [&](auto sel, dim3 grid) {
        constexpr bool S = decltype(sel)::value;
        if (a.g.nkeys == 1) hipLaunchKernelGGL((group_sum_kernel<1, S>), grid, dim3(BLOCK), 0, stream, a.g);
        else hipLaunchKernelGGL((group_sum_kernel<2, S>), grid, dim3(BLOCK), 0, stream, a.g);
    });
}

// no key column: agg_layout.hpp's scalar grid (scalar_grid_of: SCALAR_RESIDENT workgroups per compute unit)
int hj_launch_agg_group(const AggArgs &a, int cus, hipStream_t stream)
{
    using namespace hj_group;
    if (a.g.nkeys == 0)
        return grouped_launch(a, 0, 0, hj_agg::SCALAR_BLOCK, cus, hj_agg::SCALAR_RESIDENT, [&](auto sel, dim3 grid) {
            hipLaunchKernelGGL((agg_scalar_kernel<decltype(sel)::value>), grid, dim3(hj_agg::SCALAR_BLOCK), 0, stream, a);
        });
    return grouped_launch(a, 1, MAX_KEYS, BLOCK, cus, 1, [&](auto sel, dim3 grid) {
        constexpr bool S = decltype(sel)::value;
        if (a.g.nkeys == 1) hipLaunchKernelGGL((agg_group_kernel<1, S>), grid, dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((agg_group_kernel<2, S>), grid, dim3(BLOCK), 0, stream, a);
    });
}

int hj_launch_wide_group(const WideArgs &a, int cus, hipStream_t stream)
{
    using namespace hj_wide;
    return grouped_launch(a, MIN_KEYS, MAX_KEYS, BLOCK, cus, 1, [&](auto sel, dim3 grid) {
        constexpr bool S = decltype(sel)::value;
        if (a.g.nkeys == 3) hipLaunchKernelGGL((wide_group_kernel<3, S>), grid, dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((wide_group_kernel<4, S>), grid, dim3(BLOCK), 0, stream, a);
    });
}

// The emit launches' check and grid: one lane per slot of the merge table - `extra`: and of tuple 0's behind them -, eight workgroups per
// compute unit at the most
template <class Args, class Launch>
static int group_emit_launch(const Args &e, uint32_t min_keys, uint32_t max_keys, u64 extra, int cus, Launch launch)
{
    const auto &g = e.g;
    if (!g.merge || !g.d_ngroups || g.nkeys < min_keys || g.nkeys > max_keys || g.nvals > hj_agg::MAX_AGGS || (g.slots & (g.slots - 1)) || !g.slots || cus < 1) return HJGPU_EINVAL;
    for (uint32_t c = 0; c < g.nkeys; ++c) if (!g.keys_out[c]) return HJGPU_EINVAL;
    for (uint32_t c = 0; c < g.nvals; ++c) if (!g.sums_out[c] || e.fn[c] > hj_agg::MAX) return HJGPU_EINVAL;
    const u64 need = (g.slots + extra + 255) / 256;
    launch(dim3((uint32_t)std::min<u64>(need, (u64)cus * 8)));
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_group_emit(const AggEmitArgs &e, int cus, hipStream_t stream)
{
    return group_emit_launch(e, 1, hj_group::MAX_KEYS, 1, cus, [&](dim3 grid) { hipLaunchKernelGGL(group_emit_kernel, grid, dim3(256), 0, stream, e.g); });
}

int hj_launch_agg_emit(const AggEmitArgs &e, int cus, hipStream_t stream)
{
    return group_emit_launch(e, 0, hj_group::MAX_KEYS, 1, cus, [&](dim3 grid) { hipLaunchKernelGGL(agg_emit_kernel, grid, dim3(256), 0, stream, e); });
}

int hj_launch_wide_emit(const WideEmitArgs &e, int cus, hipStream_t stream)
{
    return group_emit_launch(e, hj_wide::MIN_KEYS, hj_wide::MAX_KEYS, 0, cus, [&](dim3 grid) { hipLaunchKernelGGL(wide_emit_kernel, grid, dim3(256), 0, stream, e); });
}


// ---- filter (hjgpu_filter_selected; DESIGN.md section 5 "Filter") -----------------------------------------------------------------------
// Range predicates over columns into a bitmap: row i passes when it is selected and, for every p < NPREDS, filter_layout.hpp's passes()
// holds on cols[p][i].  One persistent grid; an iteration is BATCH wave trips of hj_lookup.hpp's layout (lane L owns rows 4 L ... 4 L + 3
// of a trip, a group of 8 lanes one word of either bitmap and one 128-byte line of every column).  The head is lookup_fetch: both trips'
// mask words (SEL), then column 0 - a group whose word is 0 loads nothing -, the nibble cut at n.  Column p >= 1 is loaded only by the
// lanes whose nibble is still not 0 behind predicates 0 ... p - 1, both trips' loads before either is tested: the caller's order is the
// evaluation order, and a column line none of whose 32 rows can still pass is never fetched.  Everything non-temporal; the last, partial
// vector of a column is loaded whole and masked, as lookup_fetch does.
// The bitmap word: lookup_leave's combine - three DPP steps OR the 8 lanes' nibbles, the group's first lane stores the word when its first
// row is below n, so the last word's high bits leave as 0 and nothing at word (n + 31) / 32 or beyond is written.  hj_lookup.hpp's IN-PLACE
// RULE holds: bits_out may be select_bits, a word is read only by the wave that stores it and before it stores it (the store depends on
// the load); neither pointer is __restrict__.  The count: popcount per lane, the wave's sum, the four waves' through 32 bytes of LDS - the
// kernel's only LDS, behind the loop -, ONE 64-bit atomic add per workgroup.  No workgroup waits for another.
__device__ __forceinline__ uint32_t filter_nibble(const uint4 &x, const hj_filter::Norm &p)
{
    return (hj_filter::passes(p, x.x) ? 1u : 0u) | (hj_filter::passes(p, x.y) ? 2u : 0u) | (hj_filter::passes(p, x.z) ? 4u : 0u) |
           (hj_filter::passes(p, x.w) ? 8u : 0u);
}

template <int NPREDS, bool SEL>
__global__ __launch_bounds__(hj_filter::BLOCK) void filter_kernel(FilterArgs a)
{
    using namespace hj_filter;
    __shared__ u64 red[BLOCK / 64];
    const uint32_t tid = threadIdx.x;
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    const uint4 *c0 = reinterpret_cast<const uint4 *>(a.cols[0]);
    u64 passed = 0;
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t nib[BATCH];
        uint4 x[BATCH];
        lookup_fetch<SEL, (int)BATCH, true>(a.select_bits, c0, v0, stride, n, nib, x);
#pragma unroll
        for (int u = 0; u < (int)BATCH; ++u) nib[u] &= filter_nibble(x[u], a.preds[0]);
#pragma unroll
        for (int p = 1; p < NPREDS; ++p) {
            const uint4 *cp = reinterpret_cast<const uint4 *>(a.cols[p]);
#pragma unroll
            for (int u = 0; u < (int)BATCH; ++u) {
                x[u] = make_uint4(0, 0, 0, 0);
                if (nib[u]) x[u] = hj_load_nt(cp + v0 + (u64)u * stride + hj_lane());      // (nib != 0 only where the vector starts below n)
            }
#pragma unroll
            for (int u = 0; u < (int)BATCH; ++u) nib[u] &= filter_nibble(x[u], a.preds[p]);
        }
#pragma unroll
        for (int u = 0; u < (int)BATCH; ++u) {
            passed += __popc(nib[u]);
            if (a.bits_out) {
                const u64 v = v0 + (u64)u * stride + hj_lane();
                // 8 lanes x 4 rows = one word: OR over each group of 8 lanes, its first lane stores (all 64 lanes are here: v0 is the wave's)
                uint32_t w = nib[u] << ((tid & 7u) * 4);
                w |= hj_dpp<0xB1>(w);                                   // quad_perm: lanes 0<->1, 2<->3
                w |= hj_dpp<0x4E>(w);                                   // quad_perm: lanes 0<->2, 1<->3
                w |= hj_dpp<0x141>(w);                                  // row_half_mirror: lane i <-> 7 - i of the group, the other quad
                // (v is a multiple of 8 in the storing lane: word v / 8 starts at row 4 v; a word whose first row is at n or beyond is not stored)
                if ((tid & 7u) == 0 && (v << 2) < n) hj_store(a.bits_out + (v >> 3), w);
            }
        }
    }
    if (a.count) {
        passed = wave_reduce_sum(passed);
        if (hj_lane() == 0) red[tid >> 6] = passed;
        __syncthreads();
        if (tid == 0) {
            u64 s = 0;
#pragma unroll
            for (uint32_t w = 0; w < BLOCK / 64; ++w) s += red[w];
            if (s) atomicAdd(a.count, s);
        }
    }
}

// filter_layout.hpp's grid, no more workgroups than the rows have wave trips for
int hj_launch_filter(const FilterArgs &a, uint32_t npreds, int cus, hipStream_t stream)
{
    using namespace hj_filter;
    if (a.n == 0) return HJGPU_OK;
    if (npreds < 1 || npreds > MAX_PREDS || (!a.bits_out && !a.count) || cus < 1) return HJGPU_EINVAL;
    uintptr_t all = (uintptr_t)a.select_bits | (uintptr_t)a.bits_out;
    for (uint32_t p = 0; p < npreds; ++p) { if (!a.cols[p]) return HJGPU_EINVAL; all |= (uintptr_t)a.cols[p]; }
    if ((all & 15) || ((uintptr_t)a.count & 7)) return HJGPU_EINVAL;
    const u64 nvec = (a.n + 3) >> 2, need = (nvec + BLOCK - 1) / BLOCK;
    const dim3 grid((uint32_t)std::min<u64>(need, (u64)grid_of(cus)));
    hj_with_bool(a.select_bits != nullptr, [&](auto sel) {
        constexpr bool S = decltype(sel)::value;
        switch (npreds) {
        case 1: hipLaunchKernelGGL((filter_kernel<1, S>), grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((filter_kernel<2, S>), grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((filter_kernel<3, S>), grid, dim3(BLOCK), 0, stream, a); break;
        default: hipLaunchKernelGGL((filter_kernel<4, S>), grid, dim3(BLOCK), 0, stream, a); break;
        }
    });
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// ---- gather by row number (hjgpu_gather_selected; DESIGN.md section 5 "Gather by row number") -------------------------------------------------
// The positional look-up whose table is an array: out[c][i] = src[c][idx[i]] for every c < NCOLS where row i is gathered - selected and
// idx[i] < src_rows, gather_layout.hpp's classify() -, HJGPU_NULL_VAL and bit 0 everywhere else.  One persistent grid; an iteration is
// BATCH wave trips of hj_lookup.hpp's layout (lane L owns rows 4 L ... 4 L + 3 of a trip, a group of 8 lanes one word of either bitmap and
// one 128-byte line of the index and of every output column).  The head is lookup_fetch with the index column in the key column's place:
// all trips' mask words (SEL), then the index vectors, non-temporal, none where a group's mask word is 0, the nibble cut at n.  Then every
// row is classified and only a gathered row forms an address - in 64 bits: 4 * idx does not fit 32 from 2^30 source rows on - and issues
// its NCOLS loads; all 4 * BATCH * NCOLS loads of the iteration are issued before the first value is used.  They are ordinary cached
// loads: the rows of a dimension are read again and again, unlike the streamed index.  A row that is not gathered issues no load, so no
// index, whatever it holds, makes the kernel read outside a source column.
// The stores are lookup_leave's pattern: one 16-byte hj_store per lane, trip and column, the last, partial vector by up to three 4-byte
// stores, and the bitmap word by three DPP steps and the group's first lane - hj_lookup.hpp's IN-PLACE RULE for bits_out == select_bits.
// The counts: popcounts per lane, the wave's sums, the four waves' through 64 bytes of LDS - the kernel's only LDS, behind the loop -, one
// 64-bit atomic add per workgroup and count word.  No workgroup waits for another.
template <int NCOLS, bool SEL>
__global__ __launch_bounds__(hj_gather::BLOCK) void gather_kernel(GatherArgs a)
{
    using namespace hj_gather;
    __shared__ u64 red[2][BLOCK / 64];
    const uint32_t tid = threadIdx.x;
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    const uint4 *i4 = reinterpret_cast<const uint4 *>(a.idx);
    u64 gathered = 0, beyond = 0;
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (tid & ~63u); v0 < nvec; v0 += stride * BATCH) {
        uint32_t nib[BATCH], hit[BATCH];
        uint4 ii[BATCH];
        uint32_t val[BATCH][NCOLS][4];
        lookup_fetch<SEL, (int)BATCH, true>(a.select_bits, i4, v0, stride, n, nib, ii);
#pragma unroll
        for (int u = 0; u < (int)BATCH; ++u) {
            const uint32_t ix[4] = {ii[u].x, ii[u].y, ii[u].z, ii[u].w};
            uint32_t bad = 0;
            hit[u] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Row r = classify((nib[u] >> j) & 1u, ix[j], a.src_rows);
                hit[u] |= (r == ROW_GATHERED ? 1u : 0u) << j;
                bad |= (r == ROW_OUT_OF_RANGE ? 1u : 0u) << j;
#pragma unroll
                for (int c = 0; c < NCOLS; ++c) val[u][c][j] = NULL_VAL;
                if (r == ROW_GATHERED) {
#pragma unroll
                    for (int c = 0; c < NCOLS; ++c) val[u][c][j] = a.src[c][(u64)ix[j]];
                }
            }
            gathered += __popc(hit[u]);
            beyond += __popc(bad);
        }
#pragma unroll
        for (int u = 0; u < (int)BATCH; ++u) {
            const u64 v = v0 + (u64)u * stride + hj_lane(), g = v << 2;
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) {
                if (g + 4 <= n) hj_store(reinterpret_cast<uint4 *>(a.out[c]) + v, make_uint4(val[u][c][0], val[u][c][1], val[u][c][2], val[u][c][3]));
                else {                                              // the last, partial vector: nothing at n and beyond is written
#pragma unroll
                    for (int j = 0; j < 3; ++j) if (g + j < n) hj_store(a.out[c] + g + j, val[u][c][j]);
                }
            }
            if (a.bits_out) {
                // 8 lanes x 4 rows = one word: OR over each group of 8 lanes, its first lane stores (all 64 lanes are here: v0 is the wave's)
                uint32_t w = hit[u] << ((tid & 7u) * 4);
                w |= hj_dpp<0xB1>(w);                                   // quad_perm: lanes 0<->1, 2<->3
                w |= hj_dpp<0x4E>(w);                                   // quad_perm: lanes 0<->2, 1<->3
                w |= hj_dpp<0x141>(w);                                  // row_half_mirror: lane i <-> 7 - i of the group, the other quad
                // (v is a multiple of 8 in the storing lane: word v / 8 starts at row 4 v; a word whose first row is at n or beyond is not stored)
                if ((tid & 7u) == 0 && g < n) hj_store(a.bits_out + (v >> 3), w);
            }
        }
    }
    if (a.counts) {
        gathered = wave_reduce_sum(gathered);
        beyond = wave_reduce_sum(beyond);
        if (hj_lane() == 0) { red[0][tid >> 6] = gathered; red[1][tid >> 6] = beyond; }
        __syncthreads();
        if (tid == 0) {
            u64 s0 = 0, s1 = 0;
#pragma unroll
            for (uint32_t w = 0; w < BLOCK / 64; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
            if (s0) atomicAdd(a.counts, s0);
            if (s1) atomicAdd(a.counts + 1, s1);
        }
    }
}

// gather_layout.hpp's grid, no more workgroups than the rows have wave trips for
int hj_launch_gather(const GatherArgs &a, uint32_t ncols, int cus, hipStream_t stream)
{
    using namespace hj_gather;
    if (a.n == 0) return HJGPU_OK;
    if (ncols < 1 || ncols > MAX_COLS || !a.idx || cus < 1) return HJGPU_EINVAL;
    uintptr_t all = (uintptr_t)a.select_bits | (uintptr_t)a.idx | (uintptr_t)a.bits_out | (uintptr_t)a.counts;
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!a.src[c] || !a.out[c]) return HJGPU_EINVAL;
        all |= (uintptr_t)a.src[c] | (uintptr_t)a.out[c];
    }
    if (all & 15) return HJGPU_EINVAL;
    const u64 nvec = (a.n + 3) >> 2, need = (nvec + BLOCK - 1) / BLOCK;
    const dim3 grid((uint32_t)std::min<u64>(need, (u64)grid_of(cus)));
    hj_with_bool(a.select_bits != nullptr, [&](auto sel) {
        constexpr bool S = decltype(sel)::value;
        switch (ncols) {
        case 1: hipLaunchKernelGGL((gather_kernel<1, S>), grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((gather_kernel<2, S>), grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((gather_kernel<3, S>), grid, dim3(BLOCK), 0, stream, a); break;
        default: hipLaunchKernelGGL((gather_kernel<4, S>), grid, dim3(BLOCK), 0, stream, a); break;
        }
    });
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// ---- wide look-up (hjgpu_lookup_wide; DESIGN.md section 5 "Wide look-up") ------------------------------------------------------------------
// The positional look-up on two to four key columns: the table, the hash and the two walks are wide_lookup_layout.hpp's.  Two launches
// behind the clear of the table, ordered by the stream; no workgroup waits for another.
// The kernels stand in the header's namespace: their symbols begin with the namespace, and "wide_" at the start of a symbol stays
// hjgpu_group_by's (tests/test_group_by_isa.py reads every such kernel as one of its own).
namespace hj_wlk {

// component j of a vector (j is a constant wherever this is called: the loops over a lane's four rows are unrolled)
__device__ __forceinline__ uint32_t comp(const uint4 &q, int j) { return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w; }

// a whole slot in one (two keys) or two (three and four keys) 16-byte loads from one line: the claim word, then the key words
template <uint32_t NKEYS>
__device__ __forceinline__ void load_slot(const Slot<NKEYS> *s, u64 &claim, uint32_t (&seen)[NKEYS])
{
    const uint4 *p = reinterpret_cast<const uint4 *>(s);
    const uint4 lo = p[0];
    claim = (u64)lo.x | ((u64)lo.y << 32);
    seen[0] = lo.z; seen[1] = lo.w;
    if constexpr (NKEYS > 2) {
        const uint4 hi = p[1];
        seen[2] = hi.x;
        if constexpr (NKEYS > 3) seen[3] = hi.y;
    }
}

// the memory of insert and find: the claim is a relaxed 64-bit compare-and-swap of agent scope (global_atomic_cmpswap_x2), the winner's
// key words leave through hj_store, two at a time, and a slot is read by plain loads - in the look-up kernel, a later launch
struct GlobalMemory {
    __device__ __forceinline__ u64 cas(u64 *p, u64 word) { return atomicCAS(p, 0ull, word); }
    __device__ __forceinline__ void store_pair(uint32_t *p, uint32_t lo, uint32_t hi) { hj_store(reinterpret_cast<u64 *>(p), (u64)lo | ((u64)hi << 32)); }
    template <uint32_t NKEYS>
    __device__ __forceinline__ void load(const Slot<NKEYS> *s, u64 &claim, uint32_t (&seen)[NKEYS]) { load_slot<NKEYS>(s, claim, seen); }
};

// The build.  A lane loads vector v of every key column and of the payload column, 16 bytes each and non-temporal (the build side is read
// once; the last, partial vector is loaded whole and cut at n), and inserts its four rows one after the other: one build row per lane and
// trip through insert's walk.  No key is compared and no slot is read; the only stores are the winners' key words.
template <int NKEYS>
__global__ __launch_bounds__(BLOCK) void wide_lookup_build_kernel(WideLookupBuildArgs a)
{
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    Slot<(uint32_t)NKEYS> *tab = reinterpret_cast<Slot<(uint32_t)NKEYS> *>(a.table);
    const u64 slots = a.slots;
    const uint4 *p4 = reinterpret_cast<const uint4 *>(a.vals);
    GlobalMemory mem;
    for (u64 v = (u64)blockIdx.x * BLOCK + threadIdx.x; v < nvec; v += stride) {
        uint4 kk[NKEYS];
#pragma unroll
        for (int c = 0; c < NKEYS; ++c) kk[c] = hj_load_nt(reinterpret_cast<const uint4 *>(a.keys[c]) + v);
        const uint4 pv = hj_load_nt(p4 + v);
        const u64 g = v << 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (g + j < n) {
                uint32_t k[NKEYS];
#pragma unroll
                for (int c = 0; c < NKEYS; ++c) k[c] = comp(kk[c], j);
                (void)insert<(uint32_t)NKEYS>(mem, tab, slots, k, comp(pv, j));
            }
        }
    }
}

// The look-up.  One persistent grid; an iteration is BATCH wave trips of hj_lookup.hpp's layout (lane L owns rows 4 L ... 4 L + 3 of a
// trip, a group of 8 lanes one word of either bitmap and one 128-byte line of every key column).  The head is lookup_fetch on key column 0:
// all trips' mask words (SEL), then the key vectors, non-temporal, none where a group's mask word is 0, the nibble cut at n.  The further
// key columns' vectors are loaded by the same lane where its nibble is not 0 - without SEL that is lookup_fetch's own gate, with SEL it
// lies inside it: a group of 8 lanes whose mask word is 0 loads no key of any column.  Then the walk of wide_lookup_layout.hpp's find for
// the lane's four rows at once: home, and round by round the slot loads of all rows still walking before the first of them is judged, so
// that four slots are in flight.  A row that is not to be looked up is never walking: it issues no table load.  slots == 0 (an empty build
// side): nobody walks.  The end of a trip is lookup_leave (the in-place rule for match_bits == select_bits is hj_lookup.hpp's), the
// aggregates hj_add_to_result's.
template <int NKEYS, bool SEL, bool VALS, bool BITS>
__global__ __launch_bounds__(BLOCK) void wide_lookup_kernel(WideLookupArgs a)
{
    constexpr uint32_t NK = (uint32_t)NKEYS;
    constexpr int NB = (int)BATCH, NW = (int)(BLOCK / 64);
    __shared__ u64 red[4][NW];
    const u64 n = a.n, nvec = (n + 3) >> 2, stride = (u64)gridDim.x * BLOCK;
    const Slot<NK> *tab = reinterpret_cast<const Slot<NK> *>(a.table);
    const u64 slots = a.slots;

    u64 acc_n = 0, acc_k = 0, acc_i = 0;
    // whole waves iterate together (the bitmaps' words need all lanes)
    for (u64 v0 = (u64)blockIdx.x * BLOCK + (threadIdx.x & ~63u); v0 < nvec; v0 += stride * NB) {
        uint32_t look[NB];
        uint4 kk[NKEYS][NB];
        lookup_fetch<SEL, NB, true>(a.select_bits, reinterpret_cast<const uint4 *>(a.keys[0]), v0, stride, n, look, kk[0]);
#pragma unroll
        for (int c = 1; c < NKEYS; ++c) {
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                kk[c][u] = make_uint4(0, 0, 0, 0);
                if (look[u] != 0u) kk[c][u] = hj_load_nt(reinterpret_cast<const uint4 *>(a.keys[c]) + (v0 + (u64)u * stride + hj_lane()));
            }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            if (v0 + (u64)u * stride >= nvec) break;                     // the wave's trip lies beyond the columns (the same for all its lanes)
            const u64 v = v0 + (u64)u * stride + hj_lane();
            const uint32_t kc[4] = {kk[0][u].x, kk[0][u].y, kk[0][u].z, kk[0][u].w};
            uint32_t res[4] = {NULL_VAL, NULL_VAL, NULL_VAL, NULL_VAL};
            uint32_t nib = 0;
            uint32_t key[4][NKEYS];
            u64 s[4];
            bool act[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < NKEYS; ++c) key[j][c] = comp(kk[c][u], j);
                act[j] = slots != 0 && ((look[u] >> j) & 1u);
                s[j] = home(hash<NK>(key[j]), slots);
            }
            while (act[0] | act[1] | act[2] | act[3]) {
                u64 claim[4];
                uint32_t seen[4][NKEYS];
#pragma unroll
                for (int j = 0; j < 4; ++j) {                           // the slots of all rows still walking in flight together
                    claim[j] = 0;
#pragma unroll
                    for (int c = 0; c < NKEYS; ++c) seen[j][c] = 0;
                    if (act[j]) load_slot<NK>(tab + s[j], claim[j], seen[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (act[j]) {
                        const Step st = judge<NK>(claim[j], seen[j], key[j]);
                        if (st == STEP_NEXT) s[j] = next(s[j], slots);
                        else {
                            if (st == STEP_HIT) { res[j] = payload_of(claim[j]); nib |= 1u << j; }
                            act[j] = false;
                        }
                    }
                }
            }
            lookup_leave<VALS, BITS>(a.vals_out, a.match_bits, n, v, kc, res, nib, acc_n, acc_k, acc_i);
        }
    }
    hj_add_to_result(red, a.result, acc_n, acc_k, 0ull, acc_i);
}
}  // namespace hj_wlk

// the build's grid: no more workgroups than the rows have vectors for
int hj_launch_wide_lookup_build(const WideLookupBuildArgs &a, uint32_t nkeys, int cus, hipStream_t stream)
{
    using namespace hj_wlk;
    if (a.n == 0) return HJGPU_OK;
    if (nkeys < MIN_KEYS || nkeys > MAX_KEYS || !a.vals || !a.table || a.slots <= a.n || cus < 1) return HJGPU_EINVAL;
    uintptr_t all = (uintptr_t)a.vals;
    for (uint32_t c = 0; c < nkeys; ++c) { if (!a.keys[c]) return HJGPU_EINVAL; all |= (uintptr_t)a.keys[c]; }
    if ((all & 15) || ((uintptr_t)a.table & 31)) return HJGPU_EINVAL;
    const u64 nvec = (a.n + 3) >> 2, need = (nvec + BLOCK - 1) / BLOCK;
    const dim3 grid((uint32_t)std::min<u64>(need, (u64)cus * BUILD_RESIDENT));
    switch (nkeys) {
    case 2: hipLaunchKernelGGL((wide_lookup_build_kernel<2>), grid, dim3(BLOCK), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((wide_lookup_build_kernel<3>), grid, dim3(BLOCK), 0, stream, a); break;
    default: hipLaunchKernelGGL((wide_lookup_build_kernel<4>), grid, dim3(BLOCK), 0, stream, a); break;
    }
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// wide_lookup_layout.hpp's grid, no more workgroups than the rows have wave trips for
int hj_launch_wide_lookup(const WideLookupArgs &a, uint32_t nkeys, int cus, hipStream_t stream)
{
    using namespace hj_wlk;
    if (a.n == 0) return HJGPU_OK;
    if (nkeys < MIN_KEYS || nkeys > MAX_KEYS || !a.result || (a.slots != 0 && !a.table) || cus < 1) return HJGPU_EINVAL;
    uintptr_t all = (uintptr_t)a.select_bits | (uintptr_t)a.vals_out | (uintptr_t)a.match_bits | (uintptr_t)a.result;
    for (uint32_t c = 0; c < nkeys; ++c) { if (!a.keys[c]) return HJGPU_EINVAL; all |= (uintptr_t)a.keys[c]; }
    if ((all & 15) || ((uintptr_t)a.table & 31)) return HJGPU_EINVAL;
    const u64 nvec = (a.n + 3) >> 2, need = (nvec + BLOCK - 1) / BLOCK;
    const dim3 grid((uint32_t)std::min<u64>(need, (u64)grid_of(cus)));
    hj_with_bool(a.select_bits != nullptr, [&](auto sel) {
        hj_with_bool(a.vals_out != nullptr, [&](auto vals) {
            hj_with_bool(a.match_bits != nullptr, [&](auto bits) {
                constexpr bool S = decltype(sel)::value, V = decltype(vals)::value, M = decltype(bits)::value;
                switch (nkeys) {
                case 2: hipLaunchKernelGGL((wide_lookup_kernel<2, S, V, M>), grid, dim3(BLOCK), 0, stream, a); break;
                case 3: hipLaunchKernelGGL((wide_lookup_kernel<3, S, V, M>), grid, dim3(BLOCK), 0, stream, a); break;
                default: hipLaunchKernelGGL((wide_lookup_kernel<4, S, V, M>), grid, dim3(BLOCK), 0, stream, a); break;
                }
            });
        });
    });
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// ---- order by (hjgpu_order_by; DESIGN.md section 5 "Order by") ------------------------------------------------------------------------------
// A least-significant-digit radix sort of a PERMUTATION of row numbers: every pass of order_layout.hpp is a stable counting sort by one
// 8-bit digit of key[perm[i]].  Both roads rank a chunk through ONE body, order_rank_chunk; no workgroup ever waits for another.

// entry k of a small kernel-argument array, k uniform but not a constant (selects: a run-time index would put the array into scratch)
template <class T, int N>
__device__ __forceinline__ T order_pick(T const (&v)[N], uint32_t k)
{
    T x = v[0];
#pragma unroll
    for (int i = 1; i < N; ++i) if (k == (uint32_t)i) x = v[i];
    return x;
}

template <int BLOCK>
struct OrderRankLds {
    uint32_t wave_hist[BLOCK / 64][hj_order::DIGITS];   // a wave's running count per digit, then its first rank among the chunk's elements of that digit
    uint32_t start[hj_order::DIGITS];                   // the chunk's elements of smaller digits
    uint32_t scan[BLOCK / 64 + 1];
};

// Rank a chunk stably by digit.  A chunk is BLOCK * ITEMS elements in wave-striped order: element i of lane L of wave w stands at
// position w * 64 * ITEMS + i * 64 + L.  rank[i] = the elements of a smaller digit + the elements of the same digit at an earlier
// position; an invalid element has no rank and counts nowhere.  Inside a wave and step the lanes of one digit find each other by eight
// ballots (peers); all of them read the wave's count of the digit before the first of them adds their number to it - a wave's LDS
// instructions are performed in the order they were issued.  Thread d < 256 then owns digit d: it turns the waves' counts into their
// exclusive prefix, and a scan over the digits gives the chunk's; its count and first rank come back in my_count / my_start.
// Every thread of the workgroup calls it; four workgroup barriers.  BLOCK >= 256.
template <int BLOCK, int ITEMS>
__device__ __forceinline__ void order_rank_chunk(OrderRankLds<BLOCK> &s, const uint32_t (&dig)[ITEMS], const bool (&valid)[ITEMS],
                                                 uint32_t (&rank)[ITEMS], uint32_t &my_count, uint32_t &my_start)
{
    static_assert(BLOCK >= (int)hj_order::DIGITS && BLOCK % 64 == 0, "a thread per digit");
    constexpr int NW = BLOCK / 64;
    const uint32_t wave = threadIdx.x >> 6, lane = hj_lane();
    for (uint32_t e = lane; e < hj_order::DIGITS; e += 64) s.wave_hist[wave][e] = 0;
    compact_wave_sync();
    const u64 before = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        u64 peers = __ballot(valid[i]);
#pragma unroll
        for (uint32_t b = 0; b < hj_order::DIGIT_BITS; ++b) {
            const bool bit = (dig[i] >> b) & 1u;
            const u64 has = __ballot(bit);
            peers &= bit ? has : ~has;
        }
        const uint32_t earlier = __popcll(peers & before);
        uint32_t seen = 0;
        if (valid[i]) seen = s.wave_hist[wave][dig[i]];
        compact_wave_sync();
        if (valid[i] && earlier == 0) s.wave_hist[wave][dig[i]] = seen + (uint32_t)__popcll(peers);
        compact_wave_sync();
        rank[i] = seen + earlier;
    }
    hj_barrier_lds();
    uint32_t c = 0;
    if (threadIdx.x < hj_order::DIGITS) {
#pragma unroll
        for (int w = 0; w < NW; ++w) { const uint32_t x = s.wave_hist[w][threadIdx.x]; s.wave_hist[w][threadIdx.x] = c; c += x; }
    }
    const uint32_t first = block_exclusive_scan<BLOCK, uint32_t>(c, s.scan);
    if (threadIdx.x < hj_order::DIGITS) s.start[threadIdx.x] = first;
    my_count = c; my_start = first;
    hj_barrier_lds();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (valid[i]) rank[i] += s.start[dig[i]] + s.wave_hist[wave][dig[i]];
}

// The LDS road: ONE workgroup.  Thread t turns the mask's byte of rows [8 t, 8 t + 8) into row numbers (a block scan of the popcounts: the
// selected row numbers ascending, in LDS), then every lane holds LDS_ITEMS elements of the wave-striped order: the row number and, key by key
// from the last to the first, the key's normalised word - read once per key column.  A pass ranks the chunk, every element goes to its
// rank in LDS with its key and comes back by position.  A pass in which one digit holds every row changes nothing and is skipped: thread d
// sees it in its count, the decision travels through LDS and is the same for every thread.  At the end the first min(J, limit) elements
// store their row number and fetch and store the carried columns, 256 or 512 contiguous bytes per wave instruction.
__global__ __launch_bounds__(hj_order::LDS_BLOCK) void order_lds_kernel(OrderLdsArgs a)
{
    using namespace hj_order;
    constexpr int B = (int)LDS_BLOCK, IT = (int)LDS_ITEMS;
    static_assert(LDS_ITEMS == 8, "a thread owns one byte of the mask");
    __shared__ OrderRankLds<B> s;
    __shared__ u64 skey[LDS_ROWS];
    __shared__ uint32_t sperm[LDS_ROWS];
    __shared__ uint32_t same;
    const uint32_t tid = threadIdx.x, n = a.n;
    if (tid == 0) same = 0xFFFFFFFFu;
    const uint32_t r0 = tid * 8u;
    uint32_t bits = 0;
    if (r0 < n) {
        bits = a.select_bits ? (a.select_bits[r0 >> 5] >> (r0 & 31u)) & 0xFFu : 0xFFu;
        if (n - r0 < 8u) bits &= (1u << (n - r0)) - 1u;
    }
    uint32_t at = block_exclusive_scan<B, uint32_t>((uint32_t)__popc(bits), s.scan);
    const uint32_t J = hj_uniform(s.scan[B / 64]);
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j)
        if ((bits >> j) & 1u) sperm[at++] = r0 + j;
    __syncthreads();
    const uint32_t pos0 = (tid >> 6) * (uint32_t)(IT * 64) + hj_lane();
    uint32_t p[IT];
    bool valid[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        valid[i] = pos0 + i * 64 < J;
        p[i] = valid[i] ? sperm[pos0 + i * 64] : 0u;
    }
    __syncthreads();
    uint32_t pass = 0;
    for (uint32_t k = a.nkeys; k-- > 0;) {
        const void *col = order_pick(a.keys, k);
        const uint32_t flags = order_pick(a.key_flags, k);
        u64 key[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            u64 x = 0;
            if (valid[i]) x = (flags & WIDE) ? reinterpret_cast<const u64 *>(col)[p[i]] : (u64) reinterpret_cast<const uint32_t *>(col)[p[i]];
            key[i] = norm(x, flags);
        }
        const uint32_t nd = digits_of(flags);
        for (uint32_t d = 0; d < nd; ++d, ++pass) {
            uint32_t dig[IT], rank[IT], count, first;
#pragma unroll
            for (int i = 0; i < IT; ++i) dig[i] = digit(key[i], d);
            order_rank_chunk<B, IT>(s, dig, valid, rank, count, first);
            if (tid < DIGITS && count == J) same = pass;
            hj_barrier_lds();
            if (same == pass) continue;                                 // (uniform: every thread reads the same word)
#pragma unroll
            for (int i = 0; i < IT; ++i)
                if (valid[i]) { skey[rank[i]] = key[i]; sperm[rank[i]] = p[i]; }
            hj_barrier_lds();
#pragma unroll
            for (int i = 0; i < IT; ++i)
                if (valid[i]) { key[i] = skey[pos0 + i * 64]; p[i] = sperm[pos0 + i * 64]; }
            hj_barrier_lds();
        }
    }
    if (tid == 0) hj_store(a.d_count, (u64)J);
    const uint32_t m = (u64)J < a.limit ? J : (uint32_t)a.limit;
    if (a.rows_out) {
#pragma unroll
        for (int i = 0; i < IT; ++i)
            if (pos0 + i * 64 < m) hj_store(a.rows_out + pos0 + i * 64, p[i]);
    }
    for (uint32_t c = 0; c < a.ncols; ++c) {
        const void *in = order_pick(a.in, c);
        void *out = order_pick(a.out, c);
        if ((a.wide_cols >> c) & 1u) {
            u64 x[IT];
#pragma unroll
            for (int i = 0; i < IT; ++i) x[i] = pos0 + i * 64 < m ? reinterpret_cast<const u64 *>(in)[p[i]] : 0ull;
#pragma unroll
            for (int i = 0; i < IT; ++i)
                if (pos0 + i * 64 < m) hj_store(reinterpret_cast<u64 *>(out) + pos0 + i * 64, x[i]);
        } else {
            uint32_t x[IT];
#pragma unroll
            for (int i = 0; i < IT; ++i) x[i] = pos0 + i * 64 < m ? reinterpret_cast<const uint32_t *>(in)[p[i]] : 0u;
#pragma unroll
            for (int i = 0; i < IT; ++i)
                if (pos0 + i * 64 < m) hj_store(reinterpret_cast<uint32_t *>(out) + pos0 + i * 64, x[i]);
        }
    }
}

// The device road's initial permutation under a NULL mask: perm[i] = i for i < rows in 16-byte stores (the tail by words), *d_count = count
__global__ __launch_bounds__(256) void order_iota_kernel(uint32_t *perm, u64 rows, u64 count, u64 *d_count)
{
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x, stride = (u64)gridDim.x * 256, nvec = rows >> 2;
    for (u64 v = t; v < nvec; v += stride) {
        const uint32_t r = (uint32_t)(v << 2);
        hj_store(reinterpret_cast<uint4 *>(perm) + v, make_uint4(r, r + 1u, r + 2u, r + 3u));
    }
    if (t < (rows & 3)) hj_store(perm + (nvec << 2) + t, (uint32_t)((nvec << 2) + t));
    if (t == 0) hj_store(d_count, count);
}

// the live end of range g of the current permutation: the ranges are laid out from n, the permutation holds *d_count elements
__device__ __forceinline__ u64 order_range_end(const OrderPassArgs &a, uint32_t g, u64 live)
{
    const u64 e = a.lay.end(g);
    return e < live ? e : live;
}

// a chunk's elements in wave-striped order: the row number and the pass's digit of its key (one 32-bit word of the key column per row)
template <int ITEMS>
__device__ __forceinline__ void order_load_chunk(const OrderPassArgs &a, u64 chunk0, u64 end, uint32_t (&p)[ITEMS], uint32_t (&dig)[ITEMS], bool (&valid)[ITEMS])
{
    const u64 pos0 = chunk0 + (u64)(threadIdx.x >> 6) * (ITEMS * 64) + hj_lane();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        valid[i] = pos0 + i * 64 < end;
        p[i] = valid[i] ? a.perm_in[pos0 + i * 64] : 0u;
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t w = valid[i] ? a.key_words[(u64)p[i] * a.pass.stride + a.pass.word] : 0u;
        dig[i] = hj_order::pass_digit(w, a.pass.xor_mask, a.pass.shift);
    }
}

// A pass, launch 1: workgroup g counts the digits of its range in LDS (a wave whose lanes all hold one digit adds their number once: the
// constant high bytes of a 64-bit sum), stores counts[digit * ranges + g] and adds what it has of a digit to the pass's totals.
__global__ __launch_bounds__(hj_order::BLOCK) void order_histogram_kernel(OrderPassArgs a)
{
    using namespace hj_order;
    __shared__ uint32_t hist[BLOCK / 64][DIGITS];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, g = blockIdx.x;
#pragma unroll
    for (uint32_t w = 0; w < BLOCK / 64; ++w) hist[w][tid] = 0;
    __syncthreads();
    const u64 begin = a.lay.begin(g), end = order_range_end(a, g, *a.d_count);
    for (u64 chunk0 = begin; chunk0 < end; chunk0 += CHUNK_ROWS) {
        uint32_t p[ITEMS], dig[ITEMS];
        bool valid[ITEMS];
        order_load_chunk<(int)ITEMS>(a, chunk0, end, p, dig, valid);
#pragma unroll
        for (int i = 0; i < (int)ITEMS; ++i) {
            const u64 live = __ballot(valid[i]);
            if (live == 0) continue;
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)dig[i], __ffsll((long long)live) - 1);
            if (__ballot(valid[i] && dig[i] != d0) == 0) {
                if (hj_lane() == 0) atomicAdd(&hist[wave][d0], (uint32_t)__popcll(live));
            } else if (valid[i]) atomicAdd(&hist[wave][dig[i]], 1u);
        }
    }
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (uint32_t w = 0; w < BLOCK / 64; ++w) c += hist[w][tid];
    hj_store(&a.counts[(size_t)tid * a.lay.ranges + g], c);
    if (c) atomicAdd(&a.totals[tid], c);
}

// A pass, launch 2: workgroup d scans digit d's row of the counts over the ranges, from the total of the smaller digits:
// bases[d * ranges + g] = where range g's first element of digit d goes
__global__ __launch_bounds__(256) void order_scan_kernel(OrderPassArgs a)
{
    using namespace hj_order;
    static_assert(MAX_RANGES <= 4 * 256 && DIGITS == 256, "four ranges per thread, a workgroup per digit");
    __shared__ uint32_t red[4];
    __shared__ uint32_t scan[256 / 64 + 1];
    const uint32_t tid = threadIdx.x, d = blockIdx.x, ranges = a.lay.ranges;
    uint32_t below = tid < d ? a.totals[tid] : 0u;
    below = wave_reduce_sum(below);
    if (hj_lane() == 0) red[tid >> 6] = below;
    __syncthreads();
    below = red[0] + red[1] + red[2] + red[3];
    uint32_t c[4], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        c[j] = tid * 4 + j < ranges ? a.counts[(size_t)d * ranges + tid * 4 + j] : 0u;
        sum += c[j];
    }
    uint32_t at = below + block_exclusive_scan<256, uint32_t>(sum, scan);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (tid * 4 + j < ranges) hj_store(&a.bases[(size_t)d * ranges + tid * 4 + j], at);
        at += c[j];
    }
}

// A pass, launch 3: workgroup g walks its range chunk by chunk, in order.  Thread d keeps where the range's next element of digit d goes
// (from bases, advanced by every chunk's count).  A chunk is ranked by order_rank_chunk, its row numbers go to their ranks in LDS - the
// chunk sorted by digit - and leave from there: consecutive lanes store consecutive elements, which go to consecutive addresses as long
// as the digit stays the same.  Positions are 32-bit: the permutation has at most 2^32 - 1 elements.
__global__ __launch_bounds__(hj_order::BLOCK) void order_scatter_kernel(OrderPassArgs a)
{
    using namespace hj_order;
    __shared__ OrderRankLds<(int)BLOCK> s;
    __shared__ uint32_t sorted[CHUNK_ROWS], sdig[CHUNK_ROWS];
    __shared__ uint32_t shift_of[DIGITS];               // digit d's elements: rank r of the chunk goes to position shift_of[d] + r (modulo 2^32)
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    const u64 begin = a.lay.begin(g), end = order_range_end(a, g, *a.d_count);
    uint32_t next = 0;
    if (begin < end) next = a.bases[(size_t)tid * a.lay.ranges + g];
    for (u64 chunk0 = begin; chunk0 < end; chunk0 += CHUNK_ROWS) {
        uint32_t p[ITEMS], dig[ITEMS], rank[ITEMS], count, first;
        bool valid[ITEMS];
        order_load_chunk<(int)ITEMS>(a, chunk0, end, p, dig, valid);
        order_rank_chunk<(int)BLOCK, (int)ITEMS>(s, dig, valid, rank, count, first);
        shift_of[tid] = next - first;
        next += count;
#pragma unroll
        for (int i = 0; i < (int)ITEMS; ++i)
            if (valid[i]) { sorted[rank[i]] = p[i]; sdig[rank[i]] = dig[i]; }
        hj_barrier_lds();
        const uint32_t m = end - chunk0 < CHUNK_ROWS ? (uint32_t)(end - chunk0) : CHUNK_ROWS;
        for (uint32_t r = tid; r < m; r += BLOCK) hj_store(a.perm_out + (size_t)(uint32_t)(shift_of[sdig[r]] + r), sorted[r]);
        hj_barrier_lds();
    }
}

// The last launch: for j < min(*d_count, limit), rows_out[j] = perm[j] and out[c][j] = in[c][perm[j]], 4- or 8-byte elements
__global__ __launch_bounds__(256) void order_gather_kernel(OrderGatherArgs a)
{
    const u64 live = *a.d_count, m = live < a.limit ? live : a.limit, stride = (u64)gridDim.x * 256;
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += stride) {
        const uint32_t r = a.perm[j];
        if (a.rows_out) hj_store(a.rows_out + j, r);
        for (uint32_t c = 0; c < a.ncols; ++c) {
            const void *in = order_pick(a.in, c);
            void *out = order_pick(a.out, c);
            if ((a.wide_cols >> c) & 1u) hj_store(reinterpret_cast<u64 *>(out) + j, reinterpret_cast<const u64 *>(in)[r]);
            else hj_store(reinterpret_cast<uint32_t *>(out) + j, reinterpret_cast<const uint32_t *>(in)[r]);
        }
    }
}

static bool order_aligned(std::initializer_list<const void *> ps)
{
    uintptr_t all = 0;
    for (const void *p : ps) all |= (uintptr_t)p;
    return (all & 15) == 0;
}

int hj_launch_order_lds(const OrderLdsArgs &a, hipStream_t stream)
{
    using namespace hj_order;
    if (a.n == 0 || a.n > LDS_ROWS || a.nkeys < 1 || a.nkeys > MAX_KEYS || a.ncols > MAX_COLS || !a.d_count || ((uintptr_t)a.d_count & 7)) return HJGPU_EINVAL;
    if (!order_aligned({a.select_bits, a.rows_out})) return HJGPU_EINVAL;
    for (uint32_t k = 0; k < a.nkeys; ++k) if (!a.keys[k] || !order_aligned({a.keys[k]})) return HJGPU_EINVAL;
    for (uint32_t c = 0; c < a.ncols; ++c) if (!a.in[c] || !a.out[c] || !order_aligned({a.in[c], a.out[c]})) return HJGPU_EINVAL;
    hipLaunchKernelGGL(order_lds_kernel, dim3(1), dim3(LDS_BLOCK), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_order_iota(uint32_t *perm, u64 rows, u64 count, u64 *d_count, int cus, hipStream_t stream)
{
    if ((rows && !perm) || !d_count || !order_aligned({perm}) || ((uintptr_t)d_count & 7) || cus < 1) return HJGPU_EINVAL;
    const u64 need = ((rows >> 2) + 255) / 256;
    const dim3 grid((uint32_t)std::max<u64>(1, std::min<u64>(need, (u64)cus * 8)));
    hipLaunchKernelGGL(order_iota_kernel, grid, dim3(256), 0, stream, perm, rows, count, d_count);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

static bool order_pass_ok(const OrderPassArgs &a)
{
    return a.perm_in && a.perm_out && a.perm_in != a.perm_out && a.key_words && a.d_count && a.counts && a.bases && a.totals &&
           a.lay.ranges >= 1 && a.lay.ranges <= hj_order::MAX_RANGES && a.lay.n <= 0xFFFFFFFFull && a.pass.stride >= 1 && a.pass.stride <= 2 &&
           a.pass.word < a.pass.stride && a.pass.shift < 32;
}

int hj_launch_order_histogram(const OrderPassArgs &a, hipStream_t stream)
{
    if (!order_pass_ok(a)) return HJGPU_EINVAL;
    hipLaunchKernelGGL(order_histogram_kernel, dim3(a.lay.ranges), dim3(hj_order::BLOCK), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_order_scan(const OrderPassArgs &a, hipStream_t stream)
{
    if (!order_pass_ok(a)) return HJGPU_EINVAL;
    hipLaunchKernelGGL(order_scan_kernel, dim3(hj_order::DIGITS), dim3(256), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

int hj_launch_order_scatter(const OrderPassArgs &a, hipStream_t stream)
{
    if (!order_pass_ok(a)) return HJGPU_EINVAL;
    hipLaunchKernelGGL(order_scatter_kernel, dim3(a.lay.ranges), dim3(hj_order::BLOCK), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}

// no more workgroups than min(n, limit) - the most rows there can be - has elements for
int hj_launch_order_gather(const OrderGatherArgs &a, u64 n, int cus, hipStream_t stream)
{
    if (!a.perm || !a.d_count || a.ncols > hj_order::MAX_COLS || cus < 1) return HJGPU_EINVAL;
    for (uint32_t c = 0; c < a.ncols; ++c) if (!a.in[c] || !a.out[c]) return HJGPU_EINVAL;
    const u64 most = std::min<u64>(n, a.limit);
    if (most == 0 || (a.ncols == 0 && !a.rows_out)) return HJGPU_OK;
    const dim3 grid((uint32_t)std::min<u64>((most + 255) / 256, (u64)cus * 8));
    hipLaunchKernelGGL(order_gather_kernel, grid, dim3(256), 0, stream, a);
    return hipGetLastError() == hipSuccess ? HJGPU_OK : HJGPU_EHIP;
}
