// What the passes behind an alignment run share on the device: the companion of gact_pass.hpp (included by gact_engine.hip in
// front of it).  Every pass kernel is launched with kPassBlock threads, and four idioms are stated and argued here, once:
//   block_scan_step (on wave_scan)   a one-block exclusive scan of a few values per thread: offsets out of counts
//   table_insert_best, table_find    an open-addressing table that keeps the best item of every key, and its look-up
//   wave_count, begins_from_summary  one atomicAdd per wave of the lanes a predicate holds for; where an alignment begins
// A pass kernel calls them and reads as its own rule.
#pragma once

extern "C++" {                  // (templates: not in gact_engine.hip's extern "C")
namespace gact {

constexpr int kPassBlock = 256;                   // the block of every pass kernel
constexpr int kPassWaves = kPassBlock / 64;
static_assert(kPassWaves == 4, "block_scan_step adds up four waves; the wave-per-item grids count four items a block");

// the inclusive scan of x over the wave's lanes: six steps
template <class T>
__device__ __forceinline__ T wave_scan(T x, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(x, d);
        if (lane >= d) x += up;
    }
    return x;
}

// One chunk of a one-block scan, called by all kPassBlock threads: thread t passes own[0..N), and gets before[i] = the sum
// of own[i] over the threads below t and total[i] = the sum over the whole block.  The wave scans itself with shuffles, lane
// 63 leaves the wave's sum in LDS (four words per value), and every thread adds up the waves in front of its own: two
// barriers a chunk, however many values ride along.  A value that is only summed rides along too; its `before` is ignored.
// The second barrier keeps the next chunk's sums from landing while a slower wave still reads these.  The loop over the
// chunks, with its carry, is the kernel's: its loads and stores differ.  Everything is summed in 64 bits; the kernel loads
// its values under one branch and widens them behind it, or every `k < n ? a[k] : 0` waits for its own load (measured: r18).
template <int N>
__device__ __forceinline__ void block_scan_step(const long long (&own)[N], long long (&before)[N], long long (&total)[N])
{
    __shared__ long long s_wave[N][kPassWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long upto[N];                                          // inclusive, inside the wave
    for (int i = 0; i < N; i++) upto[i] = wave_scan(own[i], lane);
    if (lane == 63)
        for (int i = 0; i < N; i++) s_wave[i][wave] = upto[i];
    __syncthreads();
    for (int i = 0; i < N; i++) {
        long long t = 0;
        for (int w = 0; w < kPassWaves; w++) {
            if (w == wave) before[i] = t + upto[i] - own[i];
            t += s_wave[i][w];
        }
        total[i] = t;
    }
    __syncthreads();
}

// atomicAdd(counter, the number of the wave's lanes with pred), by lane 0, when there is one.  Called by whole waves.
__device__ __forceinline__ void wave_count(unsigned long long *counter, bool pred)
{
    const unsigned long long m = __ballot(pred);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// murmur3's mixing of 32-bit words, and its finaliser: ids that differ in one bit, high or low, part over the whole table.
// A key's hash is hash_final of its words mixed into kHashSeed one after the other.
constexpr uint32_t kHashSeed = 0x2545f491u;
__device__ inline uint32_t hash_mix(uint32_t h, uint32_t k)
{
    k *= 0xcc9e2d51u; k = (k << 15) | (k >> 17); k *= 0x1b873593u;
    h ^= k; h = (h << 13) | (h >> 19);
    return h * 5u + 0xe6546b64u;
}
__device__ inline uint32_t hash_final(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// The best-holder table: item indices (int32, kTableEmpty everywhere at first), mask + 1 slots, a power of two >= twice the
// items that are ever inserted, linear probing from hash & mask.  The keys and what makes an item better live in the
// caller's arrays, which no kernel writes while the table is filled: same_key(j) says whether the holder j has my key,
// better(j) whether I am better than the holder j of my key (j != me), and better must be a total order inside a key.
//
// Item `me` claims an empty slot with atomicCAS, passes a slot of another key, and at a slot of its own key replaces the
// holder only while it is better than the holder.  Returns the slot the item ended at, which then holds the item or a better
// one of its key.  The argument:
//   - a slot never becomes empty again, and a CAS only puts an item where its own key or nothing was: a slot never changes
//     its key, so every item of a key ends at the same slot, the first of the key's probe sequence that was empty;
//   - at most n of the >= 2 n slots are ever taken, so an empty slot, or the key's own, comes up before the probe is round;
//   - a holder is replaced only by a better item of its key: the inner loop sees a strictly better holder every time its CAS
//     fails, and there are finitely many, so it ends.  Nothing waits for another wave: a CAS that fails has learnt the new
//     holder and goes on with it;
//   - once all have run, the holder of a key's slot is the best of the key in the total order, whichever order the atomics
//     landed in: the winner does not depend on arrival, and neither does anything read from the table afterwards.
// (The relaxed agent-scope load in front of the CAS spares the CAS at a taken slot; what it reads may be stale, never wrong:
// a slot that was seen taken stays taken, and a stale holder costs the inner loop one failed CAS.)
constexpr int kTableEmpty = -1;                   // (hipMemsetAsync 0xff)

template <class SameKey, class Better>
__device__ __forceinline__ uint32_t table_insert_best(int *table, uint32_t mask, uint32_t hash, int me, SameKey same_key, Better better)
{
    uint32_t s = hash & mask;
    for (;;) {
        int j = __hip_atomic_load(&table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (j == kTableEmpty) {
            j = atomicCAS(&table[s], kTableEmpty, me);
            if (j == kTableEmpty) break;                       // claimed
        }
        if (same_key(j)) {
            while (better(j)) {
                const int seen = atomicCAS(&table[s], j, me);
                if (seen == j) break;
                j = seen;
            }
            break;
        }
        s = (s + 1) & mask;
    }
    return s;
}

// the holder of the key, kTableEmpty: none.  The table is complete: no kernel that looks up runs beside one that inserts
template <class SameKey>
__device__ __forceinline__ int table_find(const int *__restrict__ table, uint32_t mask, uint32_t hash, SameKey same_key)
{
    uint32_t s = hash & mask;
    for (;;) {
        const int j = table[s];
        if (j == kTableEmpty || same_key(j)) return j;
        s = (s + 1) & mask;
    }
}

// Where the alignment of record r begins on its two reads when its summary s is given: the end less the columns that consume
// a base of that read: the spans gact_hip_format_paf prints (r.ab, r.bb stay at the hit where the left extension aligned nothing)
__device__ inline void begins_from_summary(const gact_overlap &r, const gact_path_summary &s, long long &ab, long long &bb)
{
    const long long m = (long long)s.n_eq + s.n_x;
    ab = (long long)r.ae - (m + s.del_bases);
    bb = (long long)r.be - (m + s.ins_bases);
}

}  // namespace gact
}  // extern "C++"
