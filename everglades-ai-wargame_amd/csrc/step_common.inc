// step_common.inc -- what every form of the step kernel shares: the LDS layout of a wavefront's 32 envs, the phase-boundary fence, the 12-key
// sorting network, numpy's pairwise sum, the observation vector store, the random_actions generator and the pair exchange.
// Included by evg_kernels.hip inside namespace evg (not a translation unit of its own).
// LPW = lanes of the wavefront that own an env side (lane = 2 * env_slot + player): 64 (32 envs per wave) or 32
// (16 envs per wave; lanes 32..63 are helpers that only join the wave-balanced phases: combat items, write-out).
template <int LPW>
struct CombatLds {
    static constexpr int DP_CAP = LPW == 64 ? 1536 : 768;   // words of the shared damage pool (worst case of LPW/2 lanes: 33 each)
    uint32_t SNAP[12][LPW];              // pre-combat snapshot of the lane's own group k:
                                         //   bit31 fights | list-order prefix of alive units << 16 | node << 12 | alive mask
    uint32_t FS[12][LPW];                // the lane's own side at node n: alive fighting units << 16 | word offset of its damage bytes in DP
    uint32_t TURN[LPW], EPI[LPW];        // per-env scalars for lanes that work on another env's item
    uint16_t W[LPW * 12];                // work list of fighting groups: owner lane | gid << 6
    uint32_t DP[DP_CAP];                 // damage pool: one byte per targeted unit index, filled with LDS atomics
};

// The Q form of the one-seat kernel (evg_step_vs_policy_smart_q), prologue only: the wave's network output and the rows decoded from it
template <int EPW>
struct SmartQLds {
    float q[EPW][NG * 5];                // Q values [env][swarm * 5 + direction], as the caller's tensor holds them
    uint2 draws[EPW];                    // smart_explore_words of each env's agent call
    int2  rows[EPW][NA];                 // {swarm, node}: the caller's orders
    int2  dirs[EPW][NA];                 // {swarm, direction}
};

template <int LPW>
struct __align__(16) StepLds {
    uint32_t G[12][LPW];                 // group words, lane-private columns (lane = env slot, player)
    uint32_t NW[12][LPW / 2];            // node words by node ID, one column per env
    union {                              // phases are disjoint in time (one wavefront per workgroup)
        CombatLds<LPW> c;
        uint32_t A[12][LPW];             // per (own side, node): capture points | units listed << 16
        int16_t  O[LPW * OBS];           // observations of the wave's envs, already in output order [env][player][105]
        SmartQLds<LPW / 2> sq;           // (Q form, before the turn's first phase)
    } u;
    LdsTables tab;                       // the per-lane-indexed constant tables (evg_device.h), copied from DevTables::lds
};

// Phase boundary inside the step kernel.  A workgroup is ONE wavefront, and the LDS executes a wavefront's instructions in
// issue order (so do the vector-memory units, per address), so a boundary needs neither s_barrier nor a wait for outstanding
// global loads/stores (what __syncthreads() would add: s_waitcnt vmcnt(0) stalls every phase behind the turn's
// observation and health stores): it only has to keep the COMPILER from moving memory accesses across it.
#define WAVE_SYNC()                                            \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        asm volatile("" ::: "memory");                         \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)

// 12-input sorting network (tools/gen_sort12.py: 42 compare-exchanges, verified with the 0-1 principle)
#define EVG_SORT12_CES(CE) \
    CE(0, 1) CE(2, 3) CE(4, 5) CE(6, 7) CE(8, 9) CE(10, 11) CE(0, 2) CE(1, 3) \
    CE(4, 6) CE(5, 7) CE(8, 10) CE(9, 11) CE(1, 2) CE(5, 6) CE(9, 10) CE(0, 4) \
    CE(1, 5) CE(2, 6) CE(3, 7) CE(2, 4) CE(3, 5) CE(1, 2) CE(3, 4) CE(5, 6) \
    CE(9, 10) CE(0, 8) CE(1, 9) CE(2, 10) CE(3, 11) CE(4, 8) CE(5, 9) CE(6, 10) \
    CE(7, 11) CE(2, 4) CE(3, 5) CE(6, 8) CE(7, 9) CE(1, 2) CE(3, 4) CE(5, 6) \
    CE(7, 8) CE(9, 10)

// numpy's pairwise summation of a short contiguous float64 vector (np.sum at server.py:481):
// ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), then the tail sequentially.
__device__ __forceinline__ double np_sum8(const double* h) {
    return ((h[0] + h[1]) + (h[2] + h[3])) + ((h[4] + h[5]) + (h[6] + h[7]));
}

// Streaming outputs.  The observation rows -- 840 of the 971 bytes a turn must write per env -- are written once and never read back by the kernel, and they
// are stored NON-TEMPORALLY: 27 KB per wavefront and turn of ordinary stores sweep the 4 MiB L2 of the wavefront's XCD between two turns of a persistent
// launch, and with them the float64 health rows of the groups that keep fighting, which the next turn reads again.  Measured (round 5, A/B on one box +
// counter passes,
// profiles/r05_a_health_row_bytes.txt): the health-row reads that reach the fabric drop by a third (FETCH_SIZE 187 -> 130 B per env-step; the fabric moves
// whole 128-byte lines, so twice that in bytes), 1 528 -> 1 421 B per env-step in all, at the same time per turn (14.62 against 14.63 us).  The recorded orders
// (7 x 8 bytes per lane) stay ordinary stores: non-temporal 8-byte stores made the launch ERRATIC (14.9 us in some runs, 19-20 us in others; round 5), and
// they are 112 bytes against 840.
typedef uint32_t evg_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void stream_store16(void* dst, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    __builtin_nontemporal_store((evg_v4u){x, y, z, w}, reinterpret_cast<evg_v4u*>(dst));
}

template <typename OT>
__device__ __forceinline__ void store_obs_vec(OT* dst, const int (&v)[16 / sizeof(OT)]);
template <>
__device__ __forceinline__ void store_obs_vec<float>(float* dst, const int (&v)[4]) {
    stream_store16(dst, __float_as_uint((float)v[0]), __float_as_uint((float)v[1]), __float_as_uint((float)v[2]), __float_as_uint((float)v[3]));
}
template <>
__device__ __forceinline__ void store_obs_vec<double>(double* dst, const int (&v)[2]) {
    const double a = (double)v[0], b = (double)v[1];
    stream_store16(dst, (uint32_t)__double2loint(a), (uint32_t)__double2hiint(a), (uint32_t)__double2loint(b), (uint32_t)__double2hiint(b));
}
template <>
__device__ __forceinline__ void store_obs_vec<int16_t>(int16_t* dst, const int (&v)[8]) {
    stream_store16(dst, (uint32_t)(v[0] & 0xFFFF) | ((uint32_t)v[1] << 16), (uint32_t)(v[2] & 0xFFFF) | ((uint32_t)v[3] << 16),
                   (uint32_t)(v[4] & 0xFFFF) | ((uint32_t)v[5] << 16), (uint32_t)(v[6] & 0xFFFF) | ((uint32_t)v[7] << 16));
}

// One draw of a partial Fisher-Yates shuffle on a nibble-packed LIST: `pool` holds the elements not yet drawn, nibble 0 = the element at the shuffle's current
// position i.  The draw takes element k = (half * n) >> 16 of the n remaining; the front element moves into its place -- which IS the swap of positions i and
// i + k of oracle/rng_spec.py's permutation -- and the front is dropped.  11 instructions per draw where two writes into a 12-nibble permutation and the
// extraction of the drawn rows afterwards cost 26 (round 5: 363 -> ~170 instructions per lane and turn for the 14 draws of a player's orders).
__device__ __forceinline__ uint32_t fy_draw(uint64_t& pool, uint32_t half, uint32_t n) {
    const uint32_t k4 = (__umul24(half, n) >> 14) & ~3u;                  // 4 k, k = (half * n) >> 16
    const uint32_t at = (uint32_t)(pool >> k4);                           // element k in the low nibble
    pool ^= (uint64_t)((at ^ (uint32_t)pool) & 15u) << k4;                // position k := front
    pool >>= 4;                                                           // drop the front
    return at & 15u;
}

// random_actions stand-in for one (env, player): 7 distinct groups of 12 and 7 distinct nodes of 1..11
// (agents/State_Machine/random_actions.py:38-46), partial Fisher-Yates.  Same contract as oracle/rng_spec.py random_action_rows.
// halves 0..6 of block 0 pick the groups, halves 0..6 of block 1 the nodes (oracle/rng_spec.py)
__device__ __forceinline__ void rows_from_blocks(const uint4 xg, const uint4 xn, int2 (&rows)[NA]);
// (with the handle's tabulated round keys: the step kernel's form)
__device__ __forceinline__ void gen_random_rows(const uint32_t (&rk)[20], uint32_t env_id, uint32_t episode, int turn, int p, int2 (&rows)[NA]) {
    rows_from_blocks(rng_block(rk, env_id, episode, RNG_ACTION, 0u, turn, 0, p, 0), rng_block(rk, env_id, episode, RNG_ACTION, 1u, turn, 0, p, 0), rows);
}
__device__ __forceinline__ void gen_random_rows(uint32_t seed_lo, uint32_t seed_hi, uint32_t env_id, uint32_t episode, int turn, int p, int2 (&rows)[NA]) {
    rows_from_blocks(rng_block(seed_lo, seed_hi, env_id, episode, RNG_ACTION, 0u, turn, 0, p, 0),
                     rng_block(seed_lo, seed_hi, env_id, episode, RNG_ACTION, 1u, turn, 0, p, 0), rows);
}
__device__ __forceinline__ void rows_from_blocks(const uint4 xg, const uint4 xn, int2 (&rows)[NA]) {
    const uint32_t wg[4] = {xg.x, xg.y, xg.z, xg.w}, wn[4] = {xn.x, xn.y, xn.z, xn.w};
    uint64_t gp = 0xBA9876543210ull;      // nibble i = i
    uint64_t np_ = 0xBA987654321ull;      // nibble i = i + 1
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const uint32_t g = fy_draw(gp, rng_half(wg, i), (uint32_t)(12 - i));
        const uint32_t n = fy_draw(np_, rng_half(wn, i), (uint32_t)(11 - i));
        rows[i] = make_int2((int)g, (int)n);
    }
}

// zero a [12][LPW] table of per-lane columns.  With all 64 lanes owning a column (LPW == 64) the table is 3 072 contiguous bytes: three
// 16-byte-per-lane stores by the whole wave instead of twelve 4-byte ones per lane (an LDS store costs a SIMD ~16 cycles whatever its width)
template <int LPW>
__device__ __forceinline__ void zero_columns12(uint32_t (*a)[LPW], int lane, bool envlane) {
    if constexpr (LPW == WG) {
        uint4* p = reinterpret_cast<uint4*>(&a[0][0]);
#pragma unroll
        for (int j = 0; j < 3; ++j) p[lane + WG * j] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        if (envlane) {
#pragma unroll
            for (int n = 0; n < 12; ++n) a[n][lane] = 0;
        }
    }
}

// Chunk hand-over checksum (chunked persistent launches, step_kernel.inc): FNV-1a-style mix over the chunk number and every state word a lane hands on.
// Not cryptography -- it has to tell "the producer's latest words" from "an older copy of some of them", which differ in at least the turn (env word).
__device__ __forceinline__ uint32_t handoff_mix(uint32_t h, uint32_t w) { return (h ^ w) * 0x01000193u; }
__device__ __forceinline__ uint32_t handoff_sum(uint32_t seq, const uint32_t (&g)[12], const uint32_t (&st)[3], const uint32_t (&nw)[3], uint32_t envw,
                                                uint32_t episode, uint32_t ep_ret_bits) {
    uint32_t h = handoff_mix(0x811C9DC5u, seq);
#pragma unroll
    for (int k = 0; k < 12; ++k) h = handoff_mix(h, g[k]);
#pragma unroll
    for (int j = 0; j < 3; ++j) h = handoff_mix(h, st[j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) h = handoff_mix(h, nw[j]);
    return handoff_mix(handoff_mix(handoff_mix(h, envw), episode), ep_ret_bits);
}

// value held by the other player's lane of the same env (lane ^ 1): one DPP quad_perm [1,0,3,2] move, no LDS round trip
__device__ __forceinline__ int xchg1(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); }

// The handle's fault word (DevState::fault, sticky) and its host-mapped mirror: the exact bits by a device atomic, "something happened" by a plain
// system-scope store the host sees after its next synchronisation without a device copy.
__device__ __forceinline__ void raise_fault(uint32_t* fault, uint32_t* seen, uint32_t bits) {
    atomicOr(fault, bits);
    __hip_atomic_store(seen, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
