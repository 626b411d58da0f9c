// logical_search.hip -- the directed search for light undetectable logical faults (qd_search_*; the definition and its numpy mirror are
// quits_amd/search.py).  A breadth-first search over states (S, o): S a sorted set of at most 8 detectors, o a mask of observables.
//
// Memory.  States are 32-byte records in ONE pool, in level order, so a level is a contiguous range and a parent is a 32-bit pool index.  The
// visited set is an open-addressing table of 32-bit words with linear probing: 0xFFFFFFFF = empty, a value below stage_base = a pool index, a
// value from stage_base up = stage_base + an index into the staging area of the chunk in flight.  The frontier is expanded in chunks: a chunk's
// candidates that reach an empty table slot are staged, the winners of the slot are then appended to the pool and their table words rewritten to
// pool indices (qd_search_append_kernel), so duplicates never take pool space and the pool count after a level is the number of distinct states.
//
// The table protocol inside the expansion kernel.  A lane that reaches an empty slot takes a staging index, writes its record there with 8-byte
// agent-scope atomic stores (write-through), waits for them (s_waitcnt vmcnt(0)) and only then publishes stage_base + index with an agent-scope
// compare-and-swap.  A lane that finds a staged index -- from its load or from its lost compare-and-swap -- reads that record with 8-byte
// agent-scope atomic loads, which are served past this CU's L1, and compares: it reads a complete record and never waits for one.  No lane spins
// on memory, every probe loop ends after table-size steps, and every pool, staging, table and found-list write is checked against the capacity
// in SearchDev: an overflow sets a flag in the counters and drops the write.  A kernel that finds a flag set on entry does nothing.
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#include <memory>

#define QD_SEARCH_THREADS 256
#define QD_SEARCH_GROUP 16                  // lanes that share a state: they stride over the faults of its row (14 .. 234 on the fixtures)
#define QD_SEARCH_FOUND_CAP 65536
#define QD_SEARCH_EMPTY 0xFFFFFFFFu
#define QD_SEARCH_DEAD 0xFFFFFFFFFFFFFFFFull // stage_slot of a staged record that lost its slot
#define QD_SEARCH_NOSET 0xFFFFFFFFFFFFFFFFull // a word of four empty detector slots

typedef unsigned long long u64;
typedef unsigned __int128 u128;
enum { CTR_POOL = 0, CTR_STAGE = 1, CTR_FOUND = 2, CTR_FLAGS = 3, CTR_CAND = 4 };

struct alignas(16) SearchRec {
    u64 w0, w1;             // detectors 0..3 and 4..7, ascending, 16 bits each from bit 0; 0xFFFF = empty
    u64 mask;
    uint32_t parent, fault;
};
static_assert(sizeof(SearchRec) == QD_SEARCH_RECORD, "a state record is 32 bytes");

struct SearchDev {
    const uint32_t *row_ptr;        // [ndet + 1] the admitted faults of every detector (CSR)
    const int32_t *row_faults;
    const uint16_t *fault_dets;     // [n][D] sorted, 0xFFFF-padded
    const u64 *fault_obs;           // [n]
    SearchRec *pool;                // [pool_cap]
    uint32_t *table;                // [table_mask + 1]
    SearchRec *stage;               // [stage_cap]
    u64 *stage_slot;                // [stage_cap] the table slot a staged record won, or QD_SEARCH_DEAD
    uint32_t *found_idx;            // [QD_SEARCH_FOUND_CAP] pool indices of the level's (empty, o) states
    u64 *ctr;                       // [QD_SEARCH_COUNTERS]
    u64 pool_cap, table_mask, stage_cap;
    uint32_t stage_base;            // 0xFFFFFFFF - stage_cap
    int ndet, n, K, D, no_increase;
};

struct qd_search {
    SearchDev d;
    DevAllocs mem;
    int device = 0;
    uint32_t max_row = 0;
    u64 front_begin = 0, front_end = 0;      // the level to expand next
    bool fresh = true;                        // the counters were read since the last launch
    hipStream_t last = nullptr;
    ~qd_search() { mem.release(); }
};

__device__ __forceinline__ u64 search_hash(u64 w0, u64 w1, u64 mask)
{
    u64 x = w0 * 0x9E3779B97F4A7C15ull ^ (w1 + 0xD6E8FEB86659FD93ull) * 0xC2B2AE3D27D4EB4Full ^ mask * 0x165667B19E3779F9ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ void search_flag(const SearchDev &a, u64 bit) { atomicOr(a.ctr + CTR_FLAGS, bit); }

// Look the state up; stage it if no level holds it yet (the protocol of the file comment).
__device__ void search_insert(const SearchDev &a, u64 w0, u64 w1, u64 mask, uint32_t parent, uint32_t fault)
{
    u64 idx = search_hash(w0, w1, mask) & a.table_mask;
    u64 mine = QD_SEARCH_DEAD, won = QD_SEARCH_DEAD;
    bool full = true;
    for (u64 probe = 0; probe <= a.table_mask; ++probe, idx = (idx + 1) & a.table_mask) {
        uint32_t v = __hip_atomic_load(a.table + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == QD_SEARCH_EMPTY) {
            if (mine == QD_SEARCH_DEAD) {
                const u64 s = atomicAdd(a.ctr + CTR_STAGE, 1ull);
                if (s >= a.stage_cap) {
                    search_flag(a, QD_SEARCH_OVER_STAGE);
                    return;
                }
                mine = s;
                SearchRec *r = a.stage + s;
                __hip_atomic_store(&r->w0, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&r->w1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&r->mask, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                r->parent = parent;
                r->fault = fault;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the record has left this lane before its index is published
            }
            v = atomicCAS(a.table + idx, QD_SEARCH_EMPTY, a.stage_base + (uint32_t)mine);
            if (v == QD_SEARCH_EMPTY) {
                won = idx;
                full = false;
                break;
            }
        }
        u64 r0, r1, r2;
        if (v >= a.stage_base) {
            const u64 s = v - a.stage_base;
            if (s >= a.stage_cap) break;                                 // (v = 0xFFFFFFFF is handled above: not reached)
            const SearchRec *r = a.stage + s;
            r0 = __hip_atomic_load(&r->w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r1 = __hip_atomic_load(&r->w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r2 = __hip_atomic_load(&r->mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (v >= a.pool_cap) break;                                  // (a table word no kernel writes: not reached)
            const SearchRec *r = a.pool + v;                             // written by an earlier launch
            r0 = r->w0; r1 = r->w1; r2 = r->mask;
        }
        if (r0 == w0 && r1 == w1 && r2 == mask) {
            full = false;
            break;
        }
    }
    if (full) search_flag(a, QD_SEARCH_OVER_TABLE);
    if (mine != QD_SEARCH_DEAD) a.stage_slot[mine] = won;
}

// Detector d against the eight sorted slots of v: how many slots hold a smaller detector, and whether one holds d.
__device__ __forceinline__ int search_rank(u64 v0, u64 v1, uint32_t d, bool &present)
{
    int lt = 0;
    bool eq = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t s0 = (uint32_t)(v0 >> (16 * k)) & 0xFFFFu, s1 = (uint32_t)(v1 >> (16 * k)) & 0xFFFFu;
        lt += (s0 < d) + (s1 < d);
        eq |= s0 == d || s1 == d;
    }
    present = eq;
    return lt;
}

// Expansion: QD_SEARCH_GROUP lanes per frontier state, each lane the faults g, g + GROUP, ... of the row of min(S).  S xor dets(j) stays in two
// 64-bit registers: the detectors of j that S holds are removed first (pass 1), then the others are inserted in place (pass 2), so the set
// never holds more than K detectors on the way: a candidate beyond K is dropped at the insertion that would exceed it.
__global__ void __launch_bounds__(QD_SEARCH_THREADS) qd_search_expand_kernel(SearchDev a, u64 begin, u64 count)
{
    if (a.ctr[CTR_FLAGS]) return;
    const u64 t = (u64)blockIdx.x * QD_SEARCH_THREADS + threadIdx.x;
    const u64 st = t / QD_SEARCH_GROUP;
    const uint32_t g = (uint32_t)(t % QD_SEARCH_GROUP);
    if (st >= count || begin + st >= a.pool_cap) return;
    const SearchRec *rec = a.pool + begin + st;
    const u64 w0 = rec->w0, w1 = rec->w1, mask = rec->mask;
    const uint32_t first = (uint32_t)w0 & 0xFFFFu;
    if (first >= (uint32_t)a.ndet) return;                               // (empty, o): nothing to cancel
    bool dummy;
    const int n0 = search_rank(w0, w1, 0xFFFFu, dummy);                  // |S|
    u64 tried = 0;
    const uint32_t x1 = a.row_ptr[first + 1];
    for (uint32_t x = a.row_ptr[first] + g; x < x1; x += QD_SEARCH_GROUP) {
        const int j = a.row_faults[x];
        if (j < 0 || j >= a.n) continue;
        const uint16_t *fd = a.fault_dets + (size_t)j * a.D;
        u128 v = ((u128)w1 << 64) | w0;
        int cnt = n0;
        uint32_t hit = 0;
        for (int i = 0; i < a.D; ++i) {                                  // pass 1: remove what S holds
            const uint32_t d = fd[i];
            if (d == 0xFFFFu) break;
            bool present;
            const int p = search_rank((u64)v, (u64)(v >> 64), d, present);
            if (!present) continue;
            const u128 low = ((u128)1 << (16 * p)) - 1;
            v = (v & low) | ((v >> 16) & ~low) | ((u128)0xFFFFu << 112);
            cnt -= 1;
            hit |= 1u << i;
        }
        bool ok = true;
        for (int i = 0; i < a.D; ++i) {                                  // pass 2: insert the others
            const uint32_t d = fd[i];
            if (d == 0xFFFFu) break;
            if ((hit >> i) & 1u) continue;
            if (cnt >= a.K) {
                ok = false;
                break;
            }
            bool present;
            const int p = search_rank((u64)v, (u64)(v >> 64), d, present);   // p <= cnt <= 7
            const u128 low = ((u128)1 << (16 * p)) - 1;
            v = (v & low) | ((v & ~low) << 16) | ((u128)d << (16 * p));
            cnt += 1;
        }
        if (!ok || (a.no_increase && cnt > n0)) continue;
        const u64 o = mask ^ a.fault_obs[j];
        if (cnt == 0 && o == 0) continue;
        tried += 1;
        search_insert(a, (u64)v, (u64)(v >> 64), o, (uint32_t)(begin + st), (uint32_t)j);
    }
    if (tried) atomicAdd(a.ctr + CTR_CAND, tried);
}

// Level 1: the host's records (quits_amd.search.level_one) go through the same lookup.
__global__ void __launch_bounds__(QD_SEARCH_THREADS) qd_search_seed_kernel(SearchDev a, const SearchRec *__restrict__ seed, u64 count)
{
    if (a.ctr[CTR_FLAGS]) return;
    const u64 t = (u64)blockIdx.x * QD_SEARCH_THREADS + threadIdx.x;
    if (t >= count) return;
    search_insert(a, seed[t].w0, seed[t].w1, seed[t].mask, seed[t].parent, seed[t].fault);
    atomicAdd(a.ctr + CTR_CAND, 1ull);
}

// Append a chunk's winners to the pool and point their table slots at the pool.  The order inside a level is whatever the atomic gives: it
// decides only which parent a state keeps.  A state (empty, o) goes on the found list (o != 0 by construction).
__global__ void __launch_bounds__(QD_SEARCH_THREADS) qd_search_append_kernel(SearchDev a)
{
    if (a.ctr[CTR_FLAGS] & ~(u64)QD_SEARCH_OVER_POOL) return;
    const u64 staged = a.ctr[CTR_STAGE] < a.stage_cap ? a.ctr[CTR_STAGE] : a.stage_cap;
    for (u64 i = (u64)blockIdx.x * QD_SEARCH_THREADS + threadIdx.x; i < staged; i += (u64)gridDim.x * QD_SEARCH_THREADS) {
        const u64 slot = a.stage_slot[i];
        if (slot > a.table_mask) continue;                               // QD_SEARCH_DEAD
        const u64 pos = atomicAdd(a.ctr + CTR_POOL, 1ull);
        if (pos >= a.pool_cap) {
            search_flag(a, QD_SEARCH_OVER_POOL);
            continue;
        }
        const SearchRec r = a.stage[i];
        a.pool[pos] = r;
        a.table[slot] = (uint32_t)pos;
        if (r.w0 == QD_SEARCH_NOSET && r.w1 == QD_SEARCH_NOSET) {
            const u64 f = atomicAdd(a.ctr + CTR_FOUND, 1ull);
            if (f < QD_SEARCH_FOUND_CAP) a.found_idx[f] = (uint32_t)pos;
            else search_flag(a, QD_SEARCH_OVER_FOUND);
        }
    }
}

static int search_clear(qd_search *s)
{
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemset(s->d.table, 0xFF, (size_t)(s->d.table_mask + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemset(s->d.ctr, 0, QD_SEARCH_COUNTERS * sizeof(u64)));
    s->front_begin = s->front_end = 0;
    s->fresh = true;
    return QD_OK;
}

extern "C" int qd_search_create(int32_t ndet, int32_t n, const int64_t *row_ptr, const int32_t *row_faults, const uint16_t *fault_dets,
                                const uint64_t *fault_obs, int32_t K, int32_t D, int32_t no_increase, int64_t max_states, int64_t table_size,
                                int64_t stage_states, int32_t device, qd_search **out)
{
    if (!out) return qd_fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (ndet < 1 || ndet > 65535 || n < 1) return qd_fail(QD_EINVAL, "%d detectors and %d faults: 1 .. 65535 detectors, at least one fault", ndet, n);
    if (K < 1 || K > 8 || D < 1 || D > 16) return qd_fail(QD_EINVAL, "max_event_set %d (1 .. 8) or max_fault_degree %d (1 .. 16) out of range", K, D);
    if (!row_ptr || !row_faults || !fault_dets || !fault_obs) return qd_fail(QD_EINVAL, "null argument");
    if (max_states < 1 || stage_states < 1 || table_size < 2 || (table_size & (table_size - 1)) || table_size > ((int64_t)1 << 40))
        return qd_fail(QD_EINVAL, "max_states %lld, stage_states %lld and table_size %lld (a power of two) must be positive", (long long)max_states,
                       (long long)stage_states, (long long)table_size);
    if ((u64)max_states + (u64)stage_states > 0xFFFFFFFEull)
        return qd_fail(QD_ECAPACITY, "max_states %lld + stage_states %lld: pool and staging indices share 32 bits (at most 2^32 - 2)", (long long)max_states, (long long)stage_states);
    if (row_ptr[0] != 0) return qd_fail(QD_EINVAL, "row_ptr[0] must be 0");
    uint32_t max_row = 0;
    std::vector<uint32_t> rp((size_t)ndet + 1);
    for (int i = 0; i < ndet; ++i) {
        if (row_ptr[i + 1] < row_ptr[i] || row_ptr[i + 1] > (int64_t)n * D) return qd_fail(QD_EINVAL, "row_ptr is not a CSR pointer array at row %d", i);
        max_row = std::max<uint32_t>(max_row, (uint32_t)(row_ptr[i + 1] - row_ptr[i]));
        rp[i + 1] = (uint32_t)row_ptr[i + 1];
    }
    const size_t nnz = rp[ndet];
    for (size_t x = 0; x < nnz; ++x)
        if (row_faults[x] < 0 || row_faults[x] >= n) return qd_fail(QD_EINVAL, "row_faults[%zu] = %d is no fault", x, row_faults[x]);
    for (size_t x = 0; x < (size_t)n * D; ++x)
        if (fault_dets[x] != 0xFFFFu && fault_dets[x] >= ndet) return qd_fail(QD_EINVAL, "fault_dets[%zu] = %d is no detector", x, (int)fault_dets[x]);
    if ((int64_t)max_row > stage_states) return qd_fail(QD_EINVAL, "stage_states %lld is below the longest row (%u faults)", (long long)stage_states, max_row);
    std::unique_ptr<qd_search> s(new qd_search());
    s->device = device;
    s->max_row = max_row;
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    SearchDev &d = s->d;
    d.ndet = ndet; d.n = n; d.K = K; d.D = D; d.no_increase = no_increase ? 1 : 0;
    d.pool_cap = (u64)max_states; d.table_mask = (u64)table_size - 1; d.stage_cap = (u64)stage_states;
    d.stage_base = 0xFFFFFFFFu - (uint32_t)stage_states;
    // everything the search will ever touch is allocated here: a search that does not fit fails before any launch
    if (s->mem.alloc((size_t)max_states, &d.pool) != hipSuccess || s->mem.alloc((size_t)table_size, &d.table) != hipSuccess ||
        s->mem.alloc((size_t)stage_states, &d.stage) != hipSuccess || s->mem.alloc((size_t)stage_states, &d.stage_slot) != hipSuccess ||
        s->mem.alloc((size_t)QD_SEARCH_FOUND_CAP, &d.found_idx) != hipSuccess || s->mem.alloc((size_t)QD_SEARCH_COUNTERS, &d.ctr) != hipSuccess) {
        (void)hipGetLastError();
        return qd_fail(QD_EHIP, "device allocation failed: a search of %lld states, %lld table slots and %lld staged candidates", (long long)max_states,
                       (long long)table_size, (long long)stage_states);
    }
    d.row_ptr = static_cast<const uint32_t *>(s->mem.upload(rp.data(), rp.size() * sizeof(uint32_t)));
    d.row_faults = static_cast<const int32_t *>(s->mem.upload(row_faults, nnz * sizeof(int32_t)));
    d.fault_dets = static_cast<const uint16_t *>(s->mem.upload(fault_dets, (size_t)n * D * sizeof(uint16_t)));
    d.fault_obs = static_cast<const u64 *>(s->mem.upload(fault_obs, (size_t)n * sizeof(u64)));
    if (!d.row_ptr || !d.row_faults || !d.fault_dets || !d.fault_obs) return qd_fail(QD_EHIP, "device allocation/upload failed");
    if (int rc = search_clear(s.get())) return rc;
    *out = s.release();
    return QD_OK;
}

extern "C" void qd_search_destroy(qd_search *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
}

extern "C" int qd_search_reset(qd_search *s)
{
    if (!s) return qd_fail(QD_EINVAL, "null search");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->last));
    return search_clear(s);
}

static unsigned search_append_blocks(const qd_search *s)
{
    return (unsigned)std::min<u64>((s->d.stage_cap + QD_SEARCH_THREADS - 1) / QD_SEARCH_THREADS, 4096);
}

extern "C" int qd_search_seed(qd_search *s, const void *records, int64_t count, void *stream)
{
    if (!s) return qd_fail(QD_EINVAL, "null search");
    if (count < 0 || (count > 0 && !records)) return qd_fail(QD_EINVAL, "bad seed records");
    if (s->front_end != 0 || !s->fresh) return qd_fail(QD_EINVAL, "the search has started: reset it first");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(s->device));
    s->last = st;
    s->fresh = false;
    if (count == 0) return QD_OK;
    SearchRec *d_seed = nullptr;
    HIP_TRY(hipMalloc(&d_seed, (size_t)count * sizeof(SearchRec)));
    int rc = QD_OK;
    if (hipMemcpyAsync(d_seed, records, (size_t)count * sizeof(SearchRec), hipMemcpyHostToDevice, st) != hipSuccess) rc = qd_fail(QD_EHIP, "seed upload failed");
    for (int64_t c = 0; rc == QD_OK && c < count; c += (int64_t)s->d.stage_cap) {
        const u64 cnt = std::min<u64>((u64)(count - c), s->d.stage_cap);
        if (hipMemsetAsync(s->d.ctr + CTR_STAGE, 0, sizeof(u64), st) != hipSuccess) { rc = qd_fail(QD_EHIP, "memset failed"); break; }
        hipLaunchKernelGGL(qd_search_seed_kernel, dim3((unsigned)((cnt + QD_SEARCH_THREADS - 1) / QD_SEARCH_THREADS)), dim3(QD_SEARCH_THREADS), 0, st, s->d,
                           d_seed + c, cnt);
        hipLaunchKernelGGL(qd_search_append_kernel, dim3(search_append_blocks(s)), dim3(QD_SEARCH_THREADS), 0, st, s->d);
        if (hipGetLastError() != hipSuccess) rc = qd_fail(QD_EHIP, "launch failed");
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_seed);
    return rc;
}

extern "C" int qd_search_level(qd_search *s, int64_t chunk_states, void *stream)
{
    if (!s) return qd_fail(QD_EINVAL, "null search");
    if (!s->fresh) return qd_fail(QD_EINVAL, "read the counters of the previous level first (qd_search_counters)");
    if (chunk_states < 1 || (u64)chunk_states * std::max<uint32_t>(s->max_row, 1) > s->d.stage_cap)
        return qd_fail(QD_EINVAL, "chunk_states %lld times the longest row (%u faults) exceeds the %llu staged candidates", (long long)chunk_states, s->max_row,
                       s->d.stage_cap);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(s->device));
    s->last = st;
    s->fresh = false;
    const u64 begin = s->front_begin, end = s->front_end;
    s->front_begin = end;
    HIP_TRY(hipMemsetAsync(s->d.ctr + CTR_FOUND, 0, sizeof(u64), st));
    const u64 chunk = std::min<u64>((u64)chunk_states, ((u64)1 << 31) / QD_SEARCH_GROUP * QD_SEARCH_THREADS);
    for (u64 c = begin; c < end; c += chunk) {
        const u64 cnt = std::min<u64>(chunk, end - c);
        HIP_TRY(hipMemsetAsync(s->d.ctr + CTR_STAGE, 0, sizeof(u64), st));
        const u64 blocks = (cnt * QD_SEARCH_GROUP + QD_SEARCH_THREADS - 1) / QD_SEARCH_THREADS;
        hipLaunchKernelGGL(qd_search_expand_kernel, dim3((unsigned)blocks), dim3(QD_SEARCH_THREADS), 0, st, s->d, c, cnt);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(qd_search_append_kernel, dim3(search_append_blocks(s)), dim3(QD_SEARCH_THREADS), 0, st, s->d);
        HIP_TRY(hipGetLastError());
    }
    return QD_OK;
}

extern "C" int qd_search_counters(qd_search *s, uint64_t *counters)
{
    if (!s || !counters) return qd_fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->last));
    u64 c[QD_SEARCH_COUNTERS];
    HIP_TRY(hipMemcpy(c, s->d.ctr, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < QD_SEARCH_COUNTERS; ++i) counters[i] = c[i];
    s->front_end = std::min<u64>(c[CTR_POOL], s->d.pool_cap);
    if (s->front_begin > s->front_end) s->front_begin = s->front_end;
    s->fresh = true;
    return QD_OK;
}

extern "C" int qd_search_found(qd_search *s, int64_t max, uint64_t *masks, uint32_t *indices)
{
    if (!s || !masks || !indices || max < 0) return qd_fail(QD_EINVAL, "bad argument");
    if (!s->fresh) return qd_fail(QD_EINVAL, "read the counters first (qd_search_counters)");
    HIP_TRY(hipSetDevice(s->device));
    u64 c[QD_SEARCH_COUNTERS];
    HIP_TRY(hipMemcpy(c, s->d.ctr, sizeof(c), hipMemcpyDeviceToHost));
    const u64 nf = std::min<u64>(std::min<u64>(c[CTR_FOUND], QD_SEARCH_FOUND_CAP), (u64)max);
    if ((u64)max > nf) return qd_fail(QD_EINVAL, "%lld found states asked for, the level holds %llu", (long long)max, nf);
    if (nf == 0) return QD_OK;
    HIP_TRY(hipMemcpy(indices, s->d.found_idx, nf * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (u64 i = 0; i < nf; ++i) {
        if (indices[i] >= s->front_end) return qd_fail(QD_EHIP, "found index %u is outside the pool of %llu states", indices[i], s->front_end);
        SearchRec r;
        HIP_TRY(hipMemcpy(&r, s->d.pool + indices[i], sizeof(r), hipMemcpyDeviceToHost));
        masks[i] = r.mask;
    }
    return QD_OK;
}

extern "C" int qd_search_chain(qd_search *s, uint32_t index, int32_t max_len, int32_t *faults, int32_t *len)
{
    if (!s || !faults || !len || max_len < 1) return qd_fail(QD_EINVAL, "bad argument");
    if (!s->fresh) return qd_fail(QD_EINVAL, "read the counters first (qd_search_counters)");
    HIP_TRY(hipSetDevice(s->device));
    *len = 0;
    uint32_t idx = index;
    while (idx != QD_SEARCH_EMPTY) {
        if (idx >= s->front_end) return qd_fail(QD_EINVAL, "state %u is outside the pool of %llu states", idx, s->front_end);
        if (*len >= max_len) return qd_fail(QD_EINVAL, "the parent chain of state %u is longer than %d", index, max_len);
        SearchRec r;
        HIP_TRY(hipMemcpy(&r, s->d.pool + idx, sizeof(r), hipMemcpyDeviceToHost));
        if (r.parent != QD_SEARCH_EMPTY && r.parent >= idx) return qd_fail(QD_EHIP, "state %u names the later state %u as its parent", idx, r.parent);
        faults[(*len)++] = (int32_t)r.fault;
        idx = r.parent;
    }
    return QD_OK;
}
