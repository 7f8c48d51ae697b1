// replay_kernels.inc -- the Smart_State learner's n-step replay memory (include/evg.h, evg_replay_*): agents/Smart_State/Multi_Step.py and the batch
// of DQNAgent.optimize_model on the device.  Included by evg_kernels.hip (namespace evg).
//
//   evg_replay_clear_kernel    empties the ring, sets each env's counters from the handle's state
//   evg_replay_record_kernel   one thread per (env, seat): shaped reward of the turn, n-step sums of what the turn finalises, transition counts
//   evg_replay_scan_kernel     per-record counts -> per-4-record exclusive prefix inside each 1 024-record block, and the block sums
//   evg_replay_top_kernel      one workgroup: exclusive prefix of the block sums, the total, the sample call index
//   evg_replay_draw_kernel     one thread per draw: uniform transition index -> (slot, env, seat, row) by three searches
//   evg_replay_gather_kernel   one wavefront per 4 transitions: stage the two records' features in LDS, write the 59 + 708 floats per transition
//                              with 16-byte stores (one-hot and zero blocks computed, not read)

constexpr int RP_SCAN_BLOCK = 1024;        // records per workgroup of the scan (256 threads x 4)
constexpr int RP_TPW = 4;                  // transitions per wavefront of the gather
constexpr int RP_DRAW_DOMAIN = 5;          // Philox counter word 3 of the sample draws (RNG_* of evg_rng.h use 0..4 in word 0)

// utils/reward_shaping.py: the four base functions, in float64, in the reference's order of operations
__device__ __forceinline__ double rp_shape_base(int fn, double mine, double theirs, bool done, int turn) {
    switch (fn) {
        case EVG_SHAPE_NORMALIZED_SCORE: return mine;
        case EVG_SHAPE_BASIC_REWARD: return (done && mine > theirs) ? 1.0 : 0.0;
        case EVG_SHAPE_PENALIZE_LONG_GAMES: return done ? (mine > theirs ? 100.0 : -0.1) : -0.001;
        default: return done ? (mine > theirs ? (150.0 - (double)turn) / 150.0 : -1.0) : 0.0;   // reward_short_games: 150.0 is a literal there
    }
}

// The transitions of a record: order row r counts iff its swarm is in 0..11, no earlier row names that swarm (the reference takes the FIRST row of
// each swarm: Multi_Step.py addGameToReplayMemory, `break`) and its direction is not 0 (node_moved_to = direction - 1; -1 = no action).  Bit r of
// the result.
__device__ __forceinline__ uint32_t rp_row_mask(const int32_t* __restrict__ d) {
    uint32_t seen = 0, rows = 0;
#pragma unroll
    for (int r = 0; r < NA; ++r) {
        const int sw = d[2 * r], dir = d[2 * r + 1];
        if (sw >= 0 && sw < NG && !((seen >> sw) & 1u)) {
            seen |= 1u << sw;
            if (dir != 0) rows |= 1u << r;
        }
    }
    return rows;
}

__device__ __forceinline__ const int32_t* rp_dirs(const evg_replay& m, int N, int slot, long long es) {
    return m.directions + (long long)slot * EVG_REPLAY_DIRS_STRIDE(N, m.num_seats) + es * 14;
}

__global__ void __launch_bounds__(256) evg_replay_clear_kernel(evg_replay m, int N, const uint32_t* __restrict__ env_word,
                                                               const uint32_t* __restrict__ episode, int auto_reset) {
    const long long R = (long long)m.slots * N * m.num_seats;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) {
        reinterpret_cast<int4*>(m.meta)[i] = make_int4(0, 0, 0, 0);
        reinterpret_cast<double2*>(m.reward)[i] = make_double2(0.0, 0.0);
        m.count[i] = 0;
    }
    if (i < N) {
        const uint32_t w = env_word[i];
        const int frozen = (((w >> 8) & 3u) != 0u && !auto_reset) ? 1 : 0;
        reinterpret_cast<int4*>(m.env_state)[i] = make_int4((int)(w & 0xFFu), (int)episode[i], 0, frozen);
    }
    if (i < 4) m.ctl[i] = 0ull;
}

__global__ void __launch_bounds__(256) evg_replay_record_kernel(evg_replay m, int N, long long turn, const float* __restrict__ reward_in,
                                                                const uint8_t* __restrict__ done_in, const float* __restrict__ custom_in, int auto_reset) {
    const int S = m.num_seats;
    const long long es = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // (env, seat) pair
    if (es >= (long long)N * S) return;
    const int e = (int)(es / S), p = S == 1 ? m.seat : (int)(es - (long long)e * S);
    const int slots = m.slots, n = m.n_step;
    const int slot = (int)(turn % slots);
    const long long plane = (long long)N * S;                                  // records per slot
    int4* meta = reinterpret_cast<int4*>(m.meta);
    double2* rew = reinterpret_cast<double2*>(m.reward);
    // the step has written record turn + 1's features over slot (turn + 1) % slots: whatever that slot held is gone
    const long long nxt = (long long)((turn + 1) % slots) * plane + es;
    meta[nxt] = make_int4(0, 0, 0, 0);
    m.count[nxt] = 0;
    const int4 c = reinterpret_cast<const int4*>(m.env_state)[e];              // turn, episode, records of the episode kept, frozen
    if (c.w) return;                                                           // finished without auto_reset: nothing more to record
    const bool done = done_in[e] != 0;
    double shaped;
    if (m.shaping == EVG_SHAPE_CUSTOM) {
        shaped = (double)custom_in[es];
    } else {
        const float2 rw = reinterpret_cast<const float2*>(reward_in)[e];
        const double mine = (double)(p ? rw.y : rw.x), theirs = (double)(p ? rw.x : rw.y);
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
    const long long cur = (long long)slot * plane + es;
    rew[cur] = make_double2(shaped, 0.0);
    meta[cur] = make_int4(c.x, c.y, 0, 0);
    m.count[cur] = 0;
    // record s = turn - j of this episode (j <= n < slots): its shaped reward; record turn's is `shaped`
    auto shaped_of = [&](int j) -> double { return j == 0 ? shaped : rew[(long long)((slot - j + slots) % slots) * plane + es].x; };
    auto finalise = [&](int j, int flags) {
        // Multi_Step.py getSummedReward: sum_total = r[s]; for k < n: sum_total += gamma ** k * r[s + k + 1] if that step exists, else += 0
        double sum = shaped_of(j);
        for (int k = 0; k < n; ++k) {
            if (k + 1 <= j) sum += m.gamma_pow[k] * shaped_of(j - k - 1);
            else sum += 0.0;
        }
        const int ks = (slot - j + slots) % slots;
        const long long rs = (long long)ks * plane + es;
        rew[rs].y = sum;
        meta[rs].z = flags;
        m.count[rs] = (uint8_t)__popc(rp_row_mask(rp_dirs(m, N, ks, es)));
    };
    if (c.z >= n) finalise(n, EVG_REPLAY_F_FINAL | EVG_REPLAY_F_NOT_DONE);   // its next record, n turns later, is this one
    if (done) {
        const int jmax = c.z < n - 1 ? c.z : n - 1;                         // records turn - n + 1 .. turn of the episode that are kept
        for (int j = jmax; j >= 0; --j) finalise(j, EVG_REPLAY_F_FINAL);
    }
    if (S == 1 || p == S - 1) {                                             // (both lanes of an env pair read env_state above, in one wavefront)
        reinterpret_cast<int4*>(m.env_state)[e] = done ? make_int4(0, c.y + 1, 0, auto_reset ? 0 : 1) : make_int4(c.x + 1, c.y, c.z + 1, 0);
    }
}

// exclusive prefix over a 256-thread workgroup (4 wavefronts); returns the block's total in *total
__device__ __forceinline__ int rp_block_exclusive(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    *total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(256) evg_replay_scan_kernel(evg_replay m, long long R) {
    __shared__ int lds[4];
    const long long r0 = (long long)blockIdx.x * RP_SCAN_BLOCK + 4 * threadIdx.x;
    int v = 0;
    if (r0 + 3 < R) {
        const uchar4 c = *reinterpret_cast<const uchar4*>(m.count + r0);
        v = c.x + c.y + c.z + c.w;
    } else {
        for (long long r = r0; r < R; ++r) v += m.count[r];
    }
    int total;
    const int ex = rp_block_exclusive(v, lds, &total);
    const long long g = r0 / 4, G = (R + 3) / 4;
    if (g < G) m.scan[g] = ex;
    if (threadIdx.x == 0) m.scan[G + blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive block prefix (in place), total -> ctl[2]; the call index of this sample -> ctl[3], ctl[0] + 1 -> ctl[0]
__global__ void __launch_bounds__(256) evg_replay_top_kernel(evg_replay m, long long R, int count_call) {
    __shared__ int lds[4];
    const long long G = (R + 3) / 4;
    const int nb = (int)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK);
    int* bs = m.scan + G;
    const int per = (nb + 255) / 256;
    const int lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
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

// last index i in [lo, hi) with a[i] <= t (a non-decreasing, a[lo] <= t)
__device__ __forceinline__ long long rp_search(const int* __restrict__ a, long long lo, long long hi, int t) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) evg_replay_draw_kernel(evg_replay m, int N, long long R, int batch, uint32_t seed_lo, uint32_t seed_hi,
                                                              int4* __restrict__ handles) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    const unsigned long long total = m.ctl[2], call = m.ctl[3];
    if (total == 0ull) {                       // empty memory: an invalid handle, which the gather turns into zeros
        handles[i] = make_int4(-1, -1, -1, -1);
        return;
    }
    const uint4 w = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)RP_DRAW_DOMAIN), seed_lo, seed_hi);
    const int t = (int)(((unsigned long long)w.x * total) >> 32);               // uniform in [0, total) (bias below total / 2^32)
    const long long G = (R + 3) / 4;
    const int nb = (int)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK);
    const long long b = rp_search(m.scan + G, 0, nb, t);
    const int tb = t - m.scan[G + b];
    const long long g0 = b * (RP_SCAN_BLOCK / 4), g1 = g0 + RP_SCAN_BLOCK / 4 < G ? g0 + RP_SCAN_BLOCK / 4 : G;
    const long long g = rp_search(m.scan, g0, g1, tb);
    int k = tb - m.scan[g];
    long long r = 4 * g;
    while (r + 1 < R && k >= m.count[r]) k -= m.count[r++];
    const int S = m.num_seats;
    const long long plane = (long long)N * S;
    const int slot = (int)(r / plane);
    const long long es = r - (long long)slot * plane;
    uint32_t rows = rp_row_mask(rp_dirs(m, N, slot, es));
    for (int j = 0; j < k; ++j) rows &= rows - 1u;                             // the k-th counted row
    handles[i] = make_int4(slot, (int)(es / S), (int)(es % S), rows ? (int)__builtin_ctz(rows) : -1);
}

// LDS image of one transition: the acted-on swarm row (shared 34 ++ swarm[s] 13) and the next record's features (shared 34, swarm 12 x 13)
struct RpStage {
    float cur[48];
    float nsh[36];
    float nsw[156];
};

__global__ void __launch_bounds__(256) evg_replay_gather_kernel(evg_replay m, int N, int batch, const int4* __restrict__ handles, float* __restrict__ swarm_obs,
                                                                long long* __restrict__ action, float* __restrict__ next_state, float* __restrict__ reward,
                                                                uint8_t* __restrict__ not_done) {
    __shared__ RpStage st[4][RP_TPW];
    __shared__ int info[4][RP_TPW][4];                                         // valid / not_done, swarm, cur record (es), slot
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = (blockIdx.x * 4 + wave) * RP_TPW;
    const int nq = batch - i0 < RP_TPW ? (batch - i0 > 0 ? batch - i0 : 0) : RP_TPW;     // transitions of this wavefront (0 past the batch)
    const int S = m.num_seats, slots = m.slots;
    const long long plane = (long long)N * S;
    RpStage* sg = st[wave];
    if (lane < nq) {
        const int i = i0 + lane;
        const int4 h = handles[i];
        int ok = h.x >= 0 && h.x < slots && h.y >= 0 && h.y < N && h.z >= 0 && h.z < S && h.w >= 0 && h.w < NA;
        long long es = 0, rec = 0;
        int sw = 0, dir = 1, flags = 0;
        if (ok) {
            es = (long long)h.y * S + h.z;
            rec = (long long)h.x * plane + es;
            const int32_t* d = rp_dirs(m, N, h.x, es);
            ok = m.count[rec] != 0 && ((rp_row_mask(d) >> h.w) & 1u);
            sw = d[2 * h.w];
            dir = d[2 * h.w + 1];
            flags = m.meta[4 * rec + 2];
        }
        // (all -1 is what a sample of an empty memory draws: it sets its own bit)
        if (!ok && !(h.x == -1 && h.y == -1 && h.z == -1 && h.w == -1)) atomicOr(&m.ctl[1], (unsigned long long)EVG_REPLAY_S_BAD_HANDLE);
        const int nd = ok && (flags & EVG_REPLAY_F_NOT_DONE);
        info[wave][lane][0] = ok | (nd << 1);
        info[wave][lane][1] = sw;
        info[wave][lane][2] = (int)es;
        info[wave][lane][3] = h.x;
        action[i] = ok ? (long long)dir - 1 : 0;
        reward[i] = ok ? (float)m.reward[2 * rec + 1] : 0.0f;
        not_done[i] = (uint8_t)nd;
    }
    __syncthreads();
    // stage: per transition 17 float2 (acted-on shared), 13 floats (its swarm row), 17 float2 + 39 float4 (next record) = 86 pieces
    const long long sstride = EVG_REPLAY_SHARED_STRIDE(N, S);
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int idx = lane + 64 * it;
        if (idx < nq * 86) {
            const int q = idx / 86, w = idx - 86 * q;
            const int fl = info[wave][q][0];
            const long long es = info[wave][q][2];
            const int slot = info[wave][q][3];
            const int nslot = (slot + m.n_step) % (slots > 0 ? slots : 1);
            if (w < 17) {
                if (fl & 1) reinterpret_cast<float2*>(sg[q].cur)[w] = reinterpret_cast<const float2*>(m.shared + slot * sstride + es * 34)[w];
            } else if (w < 30) {
                if (fl & 1) sg[q].cur[34 + w - 17] = m.swarm[((long long)slot * plane + es) * 156 + info[wave][q][1] * 13 + (w - 17)];
            } else if (w < 47) {
                if (fl & 2) reinterpret_cast<float2*>(sg[q].nsh)[w - 30] = reinterpret_cast<const float2*>(m.shared + nslot * sstride + es * 34)[w - 30];
            } else {
                if (fl & 2) reinterpret_cast<float4*>(sg[q].nsw)[w - 47] = reinterpret_cast<const float4*>(m.swarm + ((long long)nslot * plane + es) * 156)[w - 47];
            }
        }
    }
    __syncthreads();
    // swarm_obs rows i0 .. i0 + nq - 1: 4 rows = 236 floats = 59 float4 (16-byte aligned: i0 is a multiple of 4)
    auto obs_val = [&](int q, int col) -> float {
        const int fl = info[wave][q][0];
        if (!(fl & 1)) return 0.0f;
        if (col < 47) return sg[q].cur[col];
        return col - 47 == info[wave][q][1] ? 1.0f : 0.0f;
    };
    if (nq == RP_TPW) {
        if (lane < 59) {
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int x = 4 * lane + c, q = x / 59;
                v[c] = obs_val(q, x - 59 * q);
            }
            reinterpret_cast<float4*>(swarm_obs + (long long)i0 * 59)[lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int x = lane; x < nq * 59; x += 64) {
            const int q = x / 59;
            swarm_obs[(long long)i0 * 59 + x] = obs_val(q, x - 59 * q);
        }
    }
    // next_state: 708 floats = 177 float4 per transition; zeros where not_done = 0 (nothing read)
    float4* ns = reinterpret_cast<float4*>(next_state + (long long)i0 * 708);
    for (int x = lane; x < nq * 177; x += 64) {
        const int q = x / 177, w = x - 177 * q;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (info[wave][q][0] & 2) {
            float v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int pos = 4 * w + c, row = pos / 59, col = pos - 59 * row;
                v[c] = col < 34 ? sg[q].nsh[col] : (col < 47 ? sg[q].nsw[row * 13 + col - 34] : (col - 47 == row ? 1.0f : 0.0f));
            }
            o = make_float4(v[0], v[1], v[2], v[3]);
        }
        ns[x] = o;
    }
}

int launch_replay_clear(const DevState& S, const evg_replay& m, void* stream) {
    const long long R = (long long)m.slots * S.N * m.num_seats;
    const long long n = R > S.N ? R : S.N;
    hipLaunchKernelGGL(evg_replay_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N, S.env,
                       S.episode, S.auto_reset);
    return (int)hipGetLastError();
}

int launch_replay_record(const DevState& S, const evg_replay& m, long long turn, const float* reward, const uint8_t* done, const float* custom,
                         void* stream) {
    const long long n = (long long)S.N * m.num_seats;
    hipLaunchKernelGGL(evg_replay_record_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N, turn,
                       reward, done, custom, S.auto_reset);
    return (int)hipGetLastError();
}

int launch_replay_count(const DevState& S, const evg_replay& m, int count_call, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long R = (long long)m.slots * S.N * m.num_seats;
    hipLaunchKernelGGL(evg_replay_scan_kernel, dim3((unsigned)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK)), dim3(256), 0, s, m, R);
    hipLaunchKernelGGL(evg_replay_top_kernel, dim3(1), dim3(256), 0, s, m, R, count_call);
    return (int)hipGetLastError();
}

int launch_replay_draw(const DevState& S, const evg_replay& m, int batch, uint64_t seed, int32_t* handles, void* stream) {
    const long long R = (long long)m.slots * S.N * m.num_seats;
    hipLaunchKernelGGL(evg_replay_draw_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N, R, batch,
                       (uint32_t)seed, (uint32_t)(seed >> 32), reinterpret_cast<int4*>(handles));
    return (int)hipGetLastError();
}

int launch_replay_gather(const DevState& S, const evg_replay& m, int batch, const int32_t* handles, float* swarm_obs, int64_t* action, float* next_state,
                         float* reward, uint8_t* not_done, void* stream) {
    const int waves = (batch + RP_TPW - 1) / RP_TPW;
    hipLaunchKernelGGL(evg_replay_gather_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), m, S.N, batch,
                       reinterpret_cast<const int4*>(handles), swarm_obs, reinterpret_cast<long long*>(action), next_state, reward, not_done);
    return (int)hipGetLastError();
}
