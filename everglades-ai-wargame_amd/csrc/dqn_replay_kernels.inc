// dqn_replay_kernels.inc -- the agents/DQN family's replay memory of raw observations (include/evg_dqn_replay.h, libevg_dqnreplay.so): what
// DQNAgent.remember_game_state, SimpleMemory.ReplayMemory and the batch assembly of optimize_model do, per env.  Included by evg_kernels.hip (namespace
// evg) behind replay_kernels.inc, whose device helpers (rp_shape_base, rp_block_exclusive, rp_search, RP_DRAW_DOMAIN) it calls; that file's kernels
// are not touched.
//
//   evg_dqn_replay_clear_kernel    empties the ring's records, sets each env's counters from the handle's state
//   evg_dqn_replay_record_kernel   one thread per env: shaped reward of the turn, not_done, the valid byte (all seven rows in range), counters
//   evg_dqn_replay_scan_kernel     valid bytes -> per-4-record exclusive prefix inside each 1 024-record block, and the block sums
//   evg_dqn_replay_top_kernel      one workgroup: exclusive prefix of the block sums, the total, the sample call index
//   evg_dqn_replay_draw_kernel     one thread per draw: uniform index -> the t-th valid record in (slot, env) order by two searches and a walk
//   evg_dqn_replay_gather_kernel   one workgroup per tile of 16 transitions: resolve the handles, read the 2 x 16 source rows element by element
//                                  (coalesced, converted on load) into LDS, write state / next_state with 16-byte stores over the flat index space

constexpr int DR_TILE = EVG_DQN_REPLAY_TILE;
constexpr int DR_ROW = 105;                  // OBS_LEN

__device__ __forceinline__ bool dr_actions_valid(const int32_t* __restrict__ a) {
    bool ok = true;
#pragma unroll
    for (int r = 0; r < NA; ++r) ok = ok && a[2 * r] >= 0 && a[2 * r] < NG && a[2 * r + 1] >= 0 && a[2 * r + 1] < 11;
    return ok;
}

__global__ void __launch_bounds__(256) evg_dqn_replay_clear_kernel(evg_dqn_replay m, int N, const uint32_t* __restrict__ env_word,
                                                                   const uint32_t* __restrict__ episode, int auto_reset) {
    const long long R = (long long)m.slots * N;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) {
        reinterpret_cast<int4*>(m.meta)[i] = make_int4(0, 0, 0, 0);
        m.reward[i] = 0.0;
        m.valid[i] = 0;
    }
    if (i < N) {
        const uint32_t w = env_word[i];
        const int frozen = (((w >> 8) & 3u) != 0u && !auto_reset) ? 1 : 0;
        reinterpret_cast<int4*>(m.env_state)[i] = make_int4((int)(w & 0xFFu), (int)episode[i], 0, frozen);
    }
    if (i < 4) m.ctl[i] = 0ull;
}

__global__ void __launch_bounds__(256) evg_dqn_replay_record_kernel(evg_dqn_replay m, int N, long long turn, const float* __restrict__ reward_in,
                                                                    const uint8_t* __restrict__ done_in, const float* __restrict__ custom_in,
                                                                    int auto_reset) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int slots = m.slots;
    const int slot = (int)(turn % slots);
    int4* meta = reinterpret_cast<int4*>(m.meta);
    // the step has written turn + 1's observation over slot (turn + 1) % slots: the record that slot held is gone
    const long long nxt = (long long)((turn + 1) % slots) * N + e;
    meta[nxt] = make_int4(0, 0, 0, 0);
    m.valid[nxt] = 0;
    const int4 c = reinterpret_cast<const int4*>(m.env_state)[e];              // turn, episode, records of the episode, frozen
    if (c.w) return;                                                           // finished without auto_reset: nothing more to record
    const bool done = done_in[e] != 0;
    double shaped;
    if (m.shaping == EVG_SHAPE_CUSTOM) {
        shaped = (double)custom_in[e];
    } else {
        const float2 rw = reinterpret_cast<const float2*>(reward_in)[e];
        const double mine = (double)(m.seat ? rw.y : rw.x), theirs = (double)(m.seat ? rw.x : rw.y);
        if (m.shaping == EVG_SHAPE_TRANSITION) {
            const double game = (double)(m.episode_base + 1 + (long long)c.y);
            const double ratio = fmin(1.0, game / (double)m.transition_episodes);
            const double r1 = rp_shape_base(m.shaping_from, mine, theirs, done, c.x) * (1.0 - ratio);
            const double r2 = rp_shape_base(m.shaping_to, mine, theirs, done, c.x) * ratio;
            shaped = r1 + r2;
        } else {
            shaped = rp_shape_base(m.shaping, mine, theirs, done, c.x);
        }
    }
    const long long cur = (long long)slot * N + e;
    const bool ok = dr_actions_valid(m.actions + (long long)slot * EVG_DQN_REPLAY_ACT_STRIDE(N) + e * 14);
    m.reward[cur] = shaped;
    meta[cur] = make_int4(c.x, c.y, done ? 0 : EVG_REPLAY_F_NOT_DONE, 0);
    m.valid[cur] = ok ? 1 : 0;
    if (!ok) atomicOr(&m.ctl[1], (unsigned long long)EVG_DQN_REPLAY_S_BAD_ACTION);
    reinterpret_cast<int4*>(m.env_state)[e] = done ? make_int4(0, c.y + 1, 0, auto_reset ? 0 : 1) : make_int4(c.x + 1, c.y, c.z + 1, 0);
}

__global__ void __launch_bounds__(256) evg_dqn_replay_scan_kernel(evg_dqn_replay m, long long R) {
    __shared__ int lds[4];
    const long long r0 = (long long)blockIdx.x * RP_SCAN_BLOCK + 4 * threadIdx.x;
    int v = 0;
    if (r0 + 3 < R) {
        const uchar4 c = *reinterpret_cast<const uchar4*>(m.valid + r0);
        v = c.x + c.y + c.z + c.w;
    } else {
        for (long long r = r0; r < R; ++r) v += m.valid[r];
    }
    int total;
    const int ex = rp_block_exclusive(v, lds, &total);
    const long long g = r0 / 4, G = (R + 3) / 4;
    if (g < G) m.scan[g] = ex;
    if (threadIdx.x == 0) m.scan[G + blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive block prefix (in place), total -> ctl[2]; the call index of this sample -> ctl[3], ctl[0] + 1 -> ctl[0]
__global__ void __launch_bounds__(256) evg_dqn_replay_top_kernel(evg_dqn_replay m, long long R, int count_call) {
    __shared__ int lds[4];
    const long long G = (R + 3) / 4;
    const int nb = (int)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK);
    int* bs = m.scan + G;
    const int per = (nb + 255) / 256;
    const int lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    int v = 0;
    for (int b = lo; b < hi; ++b) v += bs[b];
    int total;
    int run = rp_block_exclusive(v, lds, &total);
    for (int b = lo; b < hi; ++b) {
        const int x = bs[b];
        bs[b] = run;
        run += x;
    }
    if (threadIdx.x == 0) {
        m.ctl[2] = (unsigned long long)total;
        if (count_call) {
            m.ctl[3] = m.ctl[0];
            m.ctl[0] = m.ctl[0] + 1ull;
            if (total == 0) m.ctl[1] |= (unsigned long long)EVG_REPLAY_S_EMPTY;
        }
    }
}

__global__ void __launch_bounds__(256) evg_dqn_replay_draw_kernel(evg_dqn_replay m, int N, long long R, int batch, uint32_t seed_lo, uint32_t seed_hi,
                                                                  int4* __restrict__ handles) {
    const unsigned long long total = m.ctl[2], call = m.ctl[3];
    const long long G = (R + 3) / 4;
    const int nb = (int)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += (long long)gridDim.x * blockDim.x) {
        if (total == 0ull) {                   // empty memory: an invalid handle, which the gather turns into zeros
            handles[i] = make_int4(-1, -1, -1, -1);
            continue;
        }
        const uint4 w = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)RP_DRAW_DOMAIN), seed_lo, seed_hi);
        const int t = (int)(((unsigned long long)w.x * total) >> 32);           // uniform in [0, total) (bias below total / 2^32)
        const long long b = rp_search(m.scan + G, 0, nb, t);
        const int tb = t - m.scan[G + b];
        const long long g0 = b * (RP_SCAN_BLOCK / 4), g1 = g0 + RP_SCAN_BLOCK / 4 < G ? g0 + RP_SCAN_BLOCK / 4 : G;
        const long long g = rp_search(m.scan, g0, g1, tb);
        int k = tb - m.scan[g];
        long long r = 4 * g;
        while (r + 1 < R && k >= m.valid[r]) k -= m.valid[r++];
        const int slot = (int)(r / N);
        handles[i] = make_int4(slot, (int)(r - (long long)slot * N), 0, 0);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) evg_dqn_replay_gather_kernel(evg_dqn_replay m, int N, int batch, int flags, const int4* __restrict__ handles,
                                                                    float* __restrict__ state, long long* __restrict__ action,
                                                                    float* __restrict__ next_state, float* __restrict__ reward,
                                                                    uint8_t* __restrict__ not_done) {
    __shared__ float tile[2][DR_TILE * DR_ROW];                                // state rows, next_state rows of the tile: 13 440 bytes
    __shared__ long long src[2][DR_TILE];                                      // element offset of the source row, -1: zeros
    const T* __restrict__ obs = reinterpret_cast<const T*>(m.obs);
    const long long sstride = EVG_DQN_REPLAY_OBS_STRIDE(N, sizeof(T)) / (long long)sizeof(T);      // elements
    const int slots = m.slots;
    const int tiles = (batch + DR_TILE - 1) / DR_TILE;
    for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const int i0 = tl * DR_TILE;
        const int nq = batch - i0 < DR_TILE ? batch - i0 : DR_TILE;
        if ((int)threadIdx.x < nq) {
            const int q = threadIdx.x, i = i0 + q;
            const int4 h = handles[i];
            bool ok = h.x >= 0 && h.x < slots && h.y >= 0 && h.y < N && h.z == 0 && h.w == 0;
            long long rec = 0;
            int fl = 0;
            if (ok) {
                rec = (long long)h.x * N + h.y;
                ok = m.valid[rec] != 0;
                fl = m.meta[4 * rec + 2];
            }
            // (all -1 is what a sample of an empty memory draws: it sets its own bit)
            if (!ok && !(h.x == -1 && h.y == -1 && h.z == -1 && h.w == -1)) atomicOr(&m.ctl[1], (unsigned long long)EVG_REPLAY_S_BAD_HANDLE);
            const bool nd = ok && (fl & EVG_REPLAY_F_NOT_DONE);
            src[0][q] = ok ? (long long)h.x * sstride + (long long)h.y * DR_ROW : -1;
            src[1][q] = ok && (nd || (flags & EVG_DQN_REPLAY_TERMINAL_NEXT)) ? (long long)((h.x + 1) % slots) * sstride + (long long)h.y * DR_ROW : -1;
            const int32_t* a = m.actions + (ok ? (long long)h.x * EVG_DQN_REPLAY_ACT_STRIDE(N) + (long long)h.y * 14 : 0);
#pragma unroll
            for (int r = 0; r < NA; ++r) action[(long long)i * NA + r] = ok ? (long long)(a[2 * r] * 11 + a[2 * r + 1]) : 0ll;
            reward[i] = ok ? (float)m.reward[rec] : 0.0f;
            not_done[i] = (uint8_t)nd;
        }
        __syncthreads();
        const int ne = nq * DR_ROW;
        for (int x = threadIdx.x; x < 2 * ne; x += 256) {
            const int which = x >= ne, y = x - which * ne;
            const int q = y / DR_ROW, col = y - q * DR_ROW;
            const long long off = src[which][q];
            tile[which][y] = off >= 0 ? (float)obs[off + col] : 0.0f;
        }
        __syncthreads();
        float* __restrict__ o0 = state + (long long)i0 * DR_ROW;                // 16-byte aligned: i0 * 105 is a multiple of 4
        float* __restrict__ o1 = next_state + (long long)i0 * DR_ROW;
        const int nu = ne / 4;
        for (int x = threadIdx.x; x < 2 * nu; x += 256) {
            const int which = x >= nu, u = x - which * nu;
            reinterpret_cast<float4*>(which ? o1 : o0)[u] = reinterpret_cast<const float4*>(tile[which])[u];
        }
        for (int y = 4 * nu + threadIdx.x; y < ne; y += 256) {                  // the batch's last, partial unit
            o0[y] = tile[0][y];
            o1[y] = tile[1][y];
        }
        __syncthreads();
    }
}

int launch_dqn_replay_clear(const DevState& S, const evg_dqn_replay& m, void* stream) {
    const long long R = (long long)m.slots * S.N;
    hipLaunchKernelGGL(evg_dqn_replay_clear_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N, S.env,
                       S.episode, S.auto_reset);
    return (int)hipGetLastError();
}

int launch_dqn_replay_record(const DevState& S, const evg_dqn_replay& m, long long turn, const float* reward, const uint8_t* done, const float* custom,
                             void* stream) {
    hipLaunchKernelGGL(evg_dqn_replay_record_kernel, dim3((unsigned)((S.N + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N,
                       turn, reward, done, custom, S.auto_reset);
    return (int)hipGetLastError();
}

int launch_dqn_replay_count(const DevState& S, const evg_dqn_replay& m, int count_call, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long R = (long long)m.slots * S.N;
    hipLaunchKernelGGL(evg_dqn_replay_scan_kernel, dim3((unsigned)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK)), dim3(256), 0, s, m, R);
    hipLaunchKernelGGL(evg_dqn_replay_top_kernel, dim3(1), dim3(256), 0, s, m, R, count_call);
    return (int)hipGetLastError();
}

int launch_dqn_replay_draw(const DevState& S, const evg_dqn_replay& m, int batch, uint64_t seed, int32_t* handles, void* stream) {
    const long long R = (long long)m.slots * S.N;
    int blocks = (batch + 255) / 256;
    if (blocks > EVG_DQN_REPLAY_DRAW_MAX_BLOCKS) blocks = EVG_DQN_REPLAY_DRAW_MAX_BLOCKS;
    hipLaunchKernelGGL(evg_dqn_replay_draw_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N, R, batch,
                       (uint32_t)seed, (uint32_t)(seed >> 32), reinterpret_cast<int4*>(handles));
    return (int)hipGetLastError();
}

int launch_dqn_replay_gather(const DevState& S, const evg_dqn_replay& m, int obs_dtype, int batch, int flags, const int32_t* handles, float* state,
                             int64_t* action, float* next_state, float* reward, uint8_t* not_done, void* stream) {
    int blocks = (batch + DR_TILE - 1) / DR_TILE;
    if (blocks > EVG_DQN_REPLAY_GATHER_MAX_BLOCKS) blocks = EVG_DQN_REPLAY_GATHER_MAX_BLOCKS;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int4* h4 = reinterpret_cast<const int4*>(handles);
    long long* act = reinterpret_cast<long long*>(action);
    if (obs_dtype == EVG_OBS_I16)
        hipLaunchKernelGGL(evg_dqn_replay_gather_kernel<int16_t>, dim3((unsigned)blocks), dim3(256), 0, s, m, S.N, batch, flags, h4, state, act, next_state,
                           reward, not_done);
    else if (obs_dtype == EVG_OBS_F64)
        hipLaunchKernelGGL(evg_dqn_replay_gather_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, s, m, S.N, batch, flags, h4, state, act, next_state,
                           reward, not_done);
    else
        hipLaunchKernelGGL(evg_dqn_replay_gather_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, m, S.N, batch, flags, h4, state, act, next_state,
                           reward, not_done);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Sampling by priority (agents/DQN/PrioritizedMemory.py sample / update_priorities over the ring above; the three documented rules of
// include/evg_replay_priority.h, restated here for one weight per record):
//
//   evg_dqn_prio_clear_kernel     zeroes the weights and stamps, wmax = 1.0f
//   evg_dqn_prio_update_kernel    one thread per handle, launched twice: phase 0 resets (weight 0, the record's stamp), phase 1 takes the maximum
//                                 (atomicMax on the bits of the weight and on wmax) -- no result depends on thread order
//   evg_dqn_prio_scan_kernel      integer weights q of the valid records -> per-4-record exclusive prefix inside each 1 024-record block, block sums of
//                                 q and of the valid bytes
//   evg_dqn_prio_top_kernel       one workgroup: exclusive prefix of the block sums, Q, the record count, the sample call index
//   evg_dqn_prio_draw_kernel      one thread per draw: t = umul64hi(u, Q) -> (slot, env) by two searches and a walk; its q, the batch's least q
//   evg_dqn_prio_weights_kernel   one thread per draw: (T q / Q) ** -beta over the batch's largest, in float64, rounded once

struct DqnPrioArgs {
    float alpha;
    float* weight;
    int32_t* stamp;
    unsigned long long* pscan;
    unsigned long long* pctl;               // {wmax bits, Q, the batch's least q, 0}
};

constexpr int DR_PDRAW_DOMAIN = 7;          // Philox counter word 3 of the prioritized draws (the uniform ones use RP_DRAW_DOMAIN)

// the stamp of the record a weight belongs to, from the record's meta {turn, episode, ...}: evg_replay_priority.h's encoding
__device__ __forceinline__ uint32_t dr_stamp(const int4 meta) { return 0x80000000u | (((uint32_t)meta.y & 0x7FFFFFu) << 8) | ((uint32_t)meta.x & 0xFFu); }

// q of a weight: floor(w * 2^(32 - e)) with frexp(wmax) = (m, e), at least 1 (w <= wmax gives q < 2^32)
__device__ __forceinline__ unsigned long long dr_q(float w, int shift) {
    const unsigned long long q = (unsigned long long)ldexp((double)w, shift);
    return q ? q : 1ull;
}

__device__ __forceinline__ int dr_qshift(float wmax) {
    int e;
    (void)frexp((double)wmax, &e);
    return 32 - e;
}

// the integer weight of valid record r: the stored weight where the stamp is the record's and the weight was updated, wmax otherwise
__device__ __forceinline__ unsigned long long dr_record_q(const evg_dqn_replay& m, const DqnPrioArgs& p, long long r, float wmax, int shift) {
    const float w = p.weight[r];
    const bool fresh = (uint32_t)p.stamp[r] == dr_stamp(reinterpret_cast<const int4*>(m.meta)[r]);
    return dr_q(fresh && w != 0.0f ? w : wmax, shift);
}

__global__ void __launch_bounds__(256) evg_dqn_prio_clear_kernel(DqnPrioArgs p, long long R) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) {
        p.weight[i] = 0.0f;
        p.stamp[i] = 0;
    }
    if (i < 4) p.pctl[i] = i == 0 ? (unsigned long long)__float_as_uint(1.0f) : 0ull;
}

__global__ void __launch_bounds__(256) evg_dqn_prio_update_kernel(evg_dqn_replay m, DqnPrioArgs p, int N, int batch, const int4* __restrict__ handles,
                                                                  const float* __restrict__ priorities, int phase) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += (long long)gridDim.x * blockDim.x) {
        const int4 h = handles[i];
        const float pr = priorities[i];
        bool ok = h.x >= 0 && h.x < m.slots && h.y >= 0 && h.y < N && h.z == 0 && h.w == 0;
        long long rec = 0;
        if (ok) {
            rec = (long long)h.x * N + h.y;
            ok = m.valid[rec] != 0;
        }
        const bool good = pr > 0.0f && pr <= 3.402823466e+38f;                 // not NaN, not infinite, not <= 0
        if (phase == 0) {
            if (!ok) atomicOr(&m.ctl[1], (unsigned long long)EVG_REPLAY_S_BAD_HANDLE);
            if (!good) atomicOr(&m.ctl[1], (unsigned long long)EVG_DQN_REPLAY_S_BAD_PRIORITY);
        }
        if (!ok || !good) continue;
        if (phase == 0) {                                                      // every racing store writes these values
            p.weight[rec] = 0.0f;
            p.stamp[rec] = (int32_t)dr_stamp(reinterpret_cast<const int4*>(m.meta)[rec]);
            continue;
        }
        float w = p.alpha == 1.0f ? pr : (p.alpha == 0.0f ? 1.0f : (float)pow((double)pr, (double)p.alpha));
        if (w < 1.17549435e-38f) w = 1.17549435e-38f;                          // FLT_MIN: a stored weight is never 0 ("never updated") or subnormal
        const uint32_t bits = __float_as_uint(w);                              // positive floats order as their bits
        atomicMax(reinterpret_cast<unsigned int*>(p.weight) + rec, bits);
        atomicMax(&p.pctl[0], (unsigned long long)bits);
    }
}

// exclusive prefix of 64-bit values over a 256-thread workgroup; the block's total in *total
__device__ __forceinline__ unsigned long long dr_block_exclusive64(unsigned long long v, unsigned long long* lds, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    unsigned long long base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    *total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + x - v;
}

// pscan layout: [G] group prefixes, [nb] block sums of q (then their exclusive prefix), [nb] block sums of the valid bytes
__global__ void __launch_bounds__(256) evg_dqn_prio_scan_kernel(evg_dqn_replay m, DqnPrioArgs p, long long R) {
    __shared__ unsigned long long lds[4];
    __shared__ int ldc[4];
    const float wmax = __uint_as_float((uint32_t)p.pctl[0]);
    const int shift = dr_qshift(wmax);
    const long long r0 = (long long)blockIdx.x * RP_SCAN_BLOCK + 4 * threadIdx.x;
    unsigned long long v = 0;
    int cnt = 0;
    for (int j = 0; j < 4; ++j) {
        const long long r = r0 + j;
        if (r < R && m.valid[r]) {
            v += dr_record_q(m, p, r, wmax, shift);
            cnt += 1;
        }
    }
    unsigned long long total;
    const unsigned long long ex = dr_block_exclusive64(v, lds, &total);
    int ctotal;
    (void)rp_block_exclusive(cnt, ldc, &ctotal);
    const long long g = r0 / 4, G = (R + 3) / 4;
    const long long nb = (R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK;
    if (g < G) p.pscan[g] = ex;
    if (threadIdx.x == 0) {
        p.pscan[G + blockIdx.x] = total;
        p.pscan[G + nb + blockIdx.x] = (unsigned long long)ctotal;
    }
}

__global__ void __launch_bounds__(256) evg_dqn_prio_top_kernel(evg_dqn_replay m, DqnPrioArgs p, long long R) {
    __shared__ unsigned long long lds[4];
    const long long G = (R + 3) / 4;
    const int nb = (int)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK);
    unsigned long long* bs = p.pscan + G;
    const unsigned long long* bc = bs + nb;
    const int per = (nb + 255) / 256;
    const int lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    unsigned long long v = 0, c = 0;
    for (int b = lo; b < hi; ++b) {
        v += bs[b];
        c += bc[b];
    }
    unsigned long long total, ctotal;
    unsigned long long run = dr_block_exclusive64(v, lds, &total);
    (void)dr_block_exclusive64(c, lds, &ctotal);
    for (int b = lo; b < hi; ++b) {
        const unsigned long long x = bs[b];
        bs[b] = run;
        run += x;
    }
    if (threadIdx.x == 0) {
        p.pctl[1] = total;
        p.pctl[2] = ~0ull;
        m.ctl[2] = ctotal;
        m.ctl[3] = m.ctl[0];
        m.ctl[0] = m.ctl[0] + 1ull;
        if (ctotal == 0ull) m.ctl[1] |= (unsigned long long)EVG_REPLAY_S_EMPTY;
    }
}

// last index i in [lo, hi) with a[i] <= t (a non-decreasing, a[lo] <= t)
__device__ __forceinline__ long long dr_search64(const unsigned long long* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) evg_dqn_prio_draw_kernel(evg_dqn_replay m, DqnPrioArgs p, int N, long long R, int batch, uint32_t seed_lo,
                                                                uint32_t seed_hi, int4* __restrict__ handles, uint32_t* __restrict__ q_out) {
    const unsigned long long T = m.ctl[2], call = m.ctl[3], Q = p.pctl[1];
    const float wmax = __uint_as_float((uint32_t)p.pctl[0]);
    const int shift = dr_qshift(wmax);
    const long long G = (R + 3) / 4;
    const long long nb = (R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += (long long)gridDim.x * blockDim.x) {
        long long rec = -1;
        unsigned long long qsel = 0;
        if (T != 0ull && Q != 0ull) {
            const uint4 w = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)DR_PDRAW_DOMAIN), seed_lo, seed_hi);
            const unsigned long long t = __umul64hi(((unsigned long long)w.x << 32) | (unsigned long long)w.y, Q);     // position in [0, Q)
            const long long b = dr_search64(p.pscan + G, 0, nb, t);
            const unsigned long long tb = t - p.pscan[G + b];
            const long long g0 = b * (RP_SCAN_BLOCK / 4), g1 = g0 + RP_SCAN_BLOCK / 4 < G ? g0 + RP_SCAN_BLOCK / 4 : G;
            const long long g = dr_search64(p.pscan, g0, g1, tb);
            unsigned long long k = tb - p.pscan[g];
            bool found = false;
            for (int j = 0; j < 4; ++j) {                                      // the group's (up to four) records; position k falls into one of them
                const long long r = 4 * g + j;
                if (r >= R || !m.valid[r] || found) continue;
                const unsigned long long q = dr_record_q(m, p, r, wmax, shift);
                rec = r;
                qsel = q;
                if (k < q) found = true;
                else k -= q;
            }
        }
        if (rec < 0) {                         // empty memory (or a group without a valid record, which holds no position): an invalid handle
            handles[i] = make_int4(-1, -1, -1, -1);
            q_out[i] = 0u;
            continue;
        }
        const int slot = (int)(rec / N);
        handles[i] = make_int4(slot, (int)(rec - (long long)slot * N), 0, 0);
        q_out[i] = (uint32_t)qsel;
        atomicMin(&p.pctl[2], qsel);
    }
}

// weights[i] holds draw i's q; the batch's largest importance weight belongs to its least q (beta >= 0)
__global__ void __launch_bounds__(256) evg_dqn_prio_weights_kernel(evg_dqn_replay m, DqnPrioArgs p, int batch, float beta, float* __restrict__ weights) {
    const unsigned long long T = m.ctl[2], Q = p.pctl[1], qmin = p.pctl[2];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t q = reinterpret_cast<const uint32_t*>(weights)[i];
        float out = 0.0f;
        if (q != 0u && T != 0ull && Q != 0ull) {
            const double t = (double)T, total = (double)Q, nb = -(double)beta;
            out = (float)(pow(t * (double)q / total, nb) / pow(t * (double)qmin / total, nb));
        }
        weights[i] = out;
    }
}

static inline DqnPrioArgs dqn_prio_args(const evg_dqn_replay_priority& p) { return DqnPrioArgs{p.alpha, p.weight, p.stamp, p.pscan, p.pctl}; }

static inline unsigned dr_batch_grid(int batch) {
    const int blocks = (batch + 255) / 256;
    return (unsigned)(blocks > EVG_DQN_REPLAY_DRAW_MAX_BLOCKS ? EVG_DQN_REPLAY_DRAW_MAX_BLOCKS : blocks);
}

int launch_dqn_replay_priority_clear(const DevState& S, const evg_dqn_replay& m, const evg_dqn_replay_priority& p, void* stream) {
    const long long R = (long long)m.slots * S.N;
    hipLaunchKernelGGL(evg_dqn_prio_clear_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dqn_prio_args(p), R);
    return (int)hipGetLastError();
}

int launch_dqn_replay_priority_update(const DevState& S, const evg_dqn_replay& m, const evg_dqn_replay_priority& p, int batch, const int32_t* handles,
                                      const float* priorities, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const DqnPrioArgs a = dqn_prio_args(p);
    for (int phase = 0; phase < 2; ++phase)
        hipLaunchKernelGGL(evg_dqn_prio_update_kernel, dim3(dr_batch_grid(batch)), dim3(256), 0, s, m, a, S.N, batch, reinterpret_cast<const int4*>(handles),
                           priorities, phase);
    return (int)hipGetLastError();
}

int launch_dqn_replay_priority_draw(const DevState& S, const evg_dqn_replay& m, const evg_dqn_replay_priority& p, int batch, uint64_t seed, float beta,
                                    int32_t* handles, float* weights, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long R = (long long)m.slots * S.N;
    const DqnPrioArgs a = dqn_prio_args(p);
    hipLaunchKernelGGL(evg_dqn_prio_scan_kernel, dim3((unsigned)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK)), dim3(256), 0, s, m, a, R);
    hipLaunchKernelGGL(evg_dqn_prio_top_kernel, dim3(1), dim3(256), 0, s, m, a, R);
    hipLaunchKernelGGL(evg_dqn_prio_draw_kernel, dim3(dr_batch_grid(batch)), dim3(256), 0, s, m, a, S.N, R, batch, (uint32_t)seed, (uint32_t)(seed >> 32),
                       reinterpret_cast<int4*>(handles), reinterpret_cast<uint32_t*>(weights));
    hipLaunchKernelGGL(evg_dqn_prio_weights_kernel, dim3(dr_batch_grid(batch)), dim3(256), 0, s, m, a, batch, beta, weights);
    return (int)hipGetLastError();
}
