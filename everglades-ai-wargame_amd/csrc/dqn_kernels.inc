// dqn_kernels.inc -- the agents/DQN family's acting turn (include/evg_dqn.h): QNetwork(105 -> h1 <= 528 -> 132) on the raw observation, inference only
// (agents/DQN/QNetwork.py: relu(fc2(relu(fc1(x))))), and the kernel that runs dqn_decode.inc's rules.  Included by evg_kernels.hip (namespace evg) after
// qnet_kernels.inc, whose helpers (qn_f4, qn_mfma, qn_wave_sync, qn_relu) and numeric contract it shares; libevg_dqn.so only.
//
//   evg_dqn_qnet_kernel<XT, G>   256 threads = 4 wavefronts, one per SIMD; a wavefront owns G groups of 16 rows per pass (a workgroup pass: 64 G rows)
//   evg_dqn_qnet_rows16_kernel<XT>   the form for few rows: the workgroup's four wavefronts share ONE group of 16 rows (see there)
//   evg_dqn_actions_kernel<X>    one env per lane: filter_actions, or (X) epsilon_greedy as a whole
//
// The weights (501 KB at h1 = 528) fit neither LDS nor registers: the hidden layer is streamed in chunks of DQ_C = 48 units (528 = 11 chunks).  Per
// chunk the workgroup stages W1's 48 rows ([48][108], 105 columns and 3 zeros) and W2's 48 columns ([144][48], 132 rows and 12 of zeros) in LDS; every
// wavefront then runs layer 1 of the chunk for its G groups -- 27 k-steps x 3 column tiles, a B fragment read from LDS once and used by the G groups --,
// writes the 16 x 48 hidden tiles (ReLU, D layout) to its own LDS tiles, reads them back in the A layout and continues layer 2: 12 k-steps x 9 output
// tiles on accumulators that live in registers from the first chunk to the last (9 tiles x 4 registers per group).  The x fragments (27 registers per
// group) are read once per pass.  The next chunk's weights are fetched into registers while the current one is computed (49 values per lane) and
// written to LDS behind a barrier, so a chunk's HBM / L2 latency is paid once per pass, not per chunk.
//
// Numerics: as qnet_kernels.inc -- a sequence of 16x16x4 MFMAs over k-steps 0, 1, 2, ... with C = the bias IS the chain acc = b[j], fmaf(W[j][k], x[k],
// acc) for k ascending.  Chunking leaves layer 2's chain as it is: chunk c continues the accumulators with k = 48 c .. 48 c + 47, chunks ascending.
// Every padded position holds an exact zero on BOTH operands, by selection: the staged weights (k >= 105, unit >= h1, output >= 132), the x fragments
// (k >= 105, row >= rows) and the hidden tile (unit >= h1: whatever its accumulator holds, NaN included, 0.0f is stored).  fma(0, 0, acc) = acc up to
// the sign of a zero, which is not part of the contract.
//
// LDS strides: 110 for W1's rows, 50 for W2's rows and the hidden tiles' -- both = 2 x odd mod 32, so the 32 lanes ds_read_b32 serves per cycle
// (16 rows or columns x 2 k) fall into 32 banks.

constexpr int DQ_IN = EVG_DQN_IN;                        // 105
constexpr int DQ_H = EVG_DQN_MAX_HIDDEN;                 // 528
constexpr int DQ_C = EVG_DQN_CHUNK, DQ_CT = DQ_C / 16;   // hidden units per chunk, its column tiles
constexpr int DQ_KX = 27, DQ_KC = DQ_C / 4;              // k-steps: layer 1 (108 columns), layer 2 per chunk
constexpr int DQ_OT = 9;                                 // output tiles (144 columns)
constexpr int DQ_W1S = 110, DQ_W2S = 50, DQ_HS = 50;     // LDS row strides
constexpr int DQ_N1 = (DQ_C * 4 * DQ_KX + 255) / 256;    // staged values per lane: W1's chunk (48 x 108 = 5 184 -> 21)
constexpr int DQ_N2 = (16 * DQ_OT * DQ_C) / 256;         // ... W2's chunk (144 x 48 = 6 912 -> 27)
static_assert(16 * DQ_OT * DQ_C == 256 * DQ_N2 && DQ_C % 16 == 0 && DQ_OUT == EVG_DQN_OUT, "the staging loops and the head");

struct DqnArgs {
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    int h1, final_relu;
    long long rows;
    const void* x;              // row r's inputs: ((const XT*)x)[x_offset + r * x_stride + 0..104]
    long long x_stride, x_offset;
    float* out;
};

// One lane's share of chunk c's weights, global -> registers -> LDS.  Every load is unconditional from a clamped, valid index (unsigned: one uniform
// base and a 32-bit lane offset per load, not a 64-bit address each), and the padded positions become exact zeros by selection where the value is
// written to LDS: a predicated load, or a selection next to it, keeps one lane mask per value alive across the memory latency (SGPR spills).
struct DqnStage {
    float w1[DQ_N1], w2[DQ_N2], b1;
};
__device__ __forceinline__ void dqn_fetch(DqnStage& s, const DqnArgs& a, int c0, int tid) {
    const int last = a.h1 - 1;
    // (opaque once per call: the 49 indices are then recomputed here -- a few hundred VALU instructions per chunk -- instead of being hoisted out of
    // the loops and kept in a hundred registers across the whole kernel)
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int it = 0; it < DQ_N1; ++it) {
        const int i = tid + 256 * it, j = i / (4 * DQ_KX), k = i - (4 * DQ_KX) * j;
        s.w1[it] = a.w1[(unsigned)(min(c0 + j, last) * DQ_IN + min(k, DQ_IN - 1))];
    }
#pragma unroll
    for (int it = 0; it < DQ_N2; ++it) {
        const int i = tid + 256 * it, o = i / DQ_C, k = i - DQ_C * o;
        s.w2[it] = a.w2[(unsigned)(min(o, DQ_OUT - 1) * a.h1 + min(c0 + k, last))];
    }
    s.b1 = a.b1[(unsigned)min(c0 + (tid & 63), last)];
}
__device__ __forceinline__ void dqn_commit(const DqnStage& s, int c0, int H1, float* __restrict__ w1s, float* __restrict__ w2s, float* __restrict__ b1s,
                                           int tid) {
    asm volatile("" : "+v"(tid));                      // (as in dqn_fetch)
#pragma unroll
    for (int it = 0; it < DQ_N1; ++it) {
        const int i = tid + 256 * it, j = i / (4 * DQ_KX), k = i - (4 * DQ_KX) * j;
        if (i < DQ_C * 4 * DQ_KX) w1s[j * DQ_W1S + k] = (c0 + j < H1 && k < DQ_IN) ? s.w1[it] : 0.0f;
    }
#pragma unroll
    for (int it = 0; it < DQ_N2; ++it) {
        const int i = tid + 256 * it, o = i / DQ_C, k = i - DQ_C * o;
        w2s[o * DQ_W2S + k] = (o < DQ_OUT && c0 + k < H1) ? s.w2[it] : 0.0f;
    }
    if (tid < DQ_C) b1s[tid] = c0 + tid < H1 ? s.b1 : 0.0f;
}

template <typename XT, int G>
__global__ void __launch_bounds__(256) evg_dqn_qnet_kernel(DqnArgs a) {
    __shared__ float w1s[DQ_C * DQ_W1S];               // W1's rows of the chunk, [48][110]
    __shared__ float w2s[16 * DQ_OT * DQ_W2S];         // W2's columns of the chunk, [144][50]
    __shared__ float b1s[DQ_C];
    __shared__ float tiles[4][G][16 * DQ_HS];          // per wavefront and group: the chunk's hidden tile, [16][50]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1;
    const int chunks = (H1 + DQ_C - 1) / DQ_C;
    const long long R = a.rows;
    constexpr int RB = 64 * G;                         // rows per workgroup pass
    const long long passes = (R + RB - 1) / RB;
    const XT* __restrict__ xin = static_cast<const XT*>(a.x) + a.x_offset;

    float b2v[DQ_OT];
#pragma unroll
    for (int o = 0; o < DQ_OT; ++o) b2v[o] = 16 * o + col < DQ_OUT ? a.b2[16 * o + col] : 0.0f;

    for (long long pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const long long rbase = pass * RB + wave * (16 * G);
        // ---- this lane's A fragments of x: lane l holds x[row l & 15][4 st + (l >> 4)] of each of its G groups, converted as x.float() does
        float xa[G][DQ_KX];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long ra = rbase + 16 * g + col;
            const bool va = ra < R;
            const XT* x = xin + (va ? ra : R - 1) * a.x_stride;       // (a clamped row and column: every load is inside the buffer)
#pragma unroll
            for (int s = 0; s < DQ_KX; ++s) {
                const int k = 4 * s + kq;
                const float v = (float)x[4 * s + 3 < DQ_IN ? k : min(k, DQ_IN - 1)];
                xa[g][s] = (va && (4 * s + 3 < DQ_IN || k < DQ_IN)) ? v : 0.0f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        DqnStage st;
        dqn_fetch(st, a, 0, tid);
        qn_f4 acc2[G][DQ_OT];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int o = 0; o < DQ_OT; ++o) acc2[g][o] = qn_f4{b2v[o], b2v[o], b2v[o], b2v[o]};

        int c = 0;                                     // (h1 >= 1: at least one chunk)
#pragma unroll 1
        do {
            const int c0 = c * DQ_C;
            __syncthreads();                           // every wavefront is done with the chunk that LDS holds
            dqn_commit(st, c0, H1, w1s, w2s, b1s, tid);
            __syncthreads();
            if (c + 1 < chunks) dqn_fetch(st, a, c0 + DQ_C, tid);      // in flight during this chunk's MFMAs
            __builtin_amdgcn_sched_barrier(0);

            // ---- layer 1 of the chunk: 3 column tiles x G groups, 27 k-steps each.  TI tiles run side by side: with the G groups that is at least
            // three independent accumulator chains (a dependent 16x16x4 MFMA issues after 40 cycles, an independent one after 32)
            constexpr int TI = G >= 3 ? 1 : DQ_CT;
#pragma unroll 1
            for (int tb = 0; tb < DQ_CT; tb += TI) {
                qn_f4 acc1[TI][G];
#pragma unroll
                for (int t = 0; t < TI; ++t) {
                    const float b = b1s[16 * (tb + t) + col];
#pragma unroll
                    for (int g = 0; g < G; ++g) acc1[t][g] = qn_f4{b, b, b, b};
                }
#pragma unroll
                for (int s = 0; s < DQ_KX; ++s)
#pragma unroll
                    for (int t = 0; t < TI; ++t) {
                        const float w = w1s[(16 * (tb + t) + col) * DQ_W1S + 4 * s + kq];
#pragma unroll
                        for (int g = 0; g < G; ++g) acc1[t][g] = qn_mfma(xa[g][s], w, acc1[t][g]);
                    }
                // ---- ReLU, D layout -> the wavefront's tiles; a unit >= h1 is an exact zero whatever its accumulator holds
#pragma unroll
                for (int t = 0; t < TI; ++t) {
                    const bool unit = c0 + 16 * (tb + t) + col < H1;
#pragma unroll
                    for (int g = 0; g < G; ++g)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            tiles[wave][g][(row0 + r) * DQ_HS + 16 * (tb + t) + col] = unit ? qn_relu(acc1[t][g][r]) : 0.0f;
                }
            }
            qn_wave_sync();
            // ---- layer 2 continued with the chunk's 48 k: 12 k-steps x 9 output tiles x G groups
            constexpr int U2 = G >= 3 ? 2 : DQ_KC;    // (four groups: 72 MFMAs per two k-steps already cover the LDS reads of the next two)
#pragma unroll U2
            for (int s = 0; s < DQ_KC; ++s) {
                float h[G];
#pragma unroll
                for (int g = 0; g < G; ++g) h[g] = tiles[wave][g][col * DQ_HS + 4 * s + kq];
#pragma unroll
                for (int o = 0; o < DQ_OT; ++o) {
                    const float w = w2s[(16 * o + col) * DQ_W2S + 4 * s + kq];
#pragma unroll
                    for (int g = 0; g < G; ++g) acc2[g][o] = qn_mfma(h[g], w, acc2[g][o]);
                }
            }
            qn_wave_sync();                            // the tiles are rewritten by the next chunk
        } while (++c < chunks);

        // ---- Q leaves the accumulators: lane l register r = [row 4 (l >> 4) + r][column 16 o + (l & 15)]
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = rbase + 16 * g + row0 + r;
                if (row < R)
#pragma unroll
                    for (int o = 0; o < DQ_OT; ++o)
                        if (16 * o + col < DQ_OUT) a.out[row * DQ_OUT + 16 * o + col] = a.final_relu ? qn_relu(acc2[g][o][r]) : acc2[g][o][r];
            }
    }
}

// The form for few rows (<= EVG_DQN_TINY_ROWS): a workgroup pass is ONE group of 16 rows, so that 4 096 rows already occupy 256 CUs, and the four
// wavefronts share the group instead of owning rows -- layer 1's three column tiles of the chunk go to wavefronts 0..2 (each the whole 27-step chain of
// its tile), the 16 x 48 hidden tile is one tile of the workgroup behind a barrier, and layer 2's nine output tiles are dealt 2, 2, 2, 3 (wavefront 3,
// idle in layer 1, takes three).  Every accumulator still sees all of k in ascending order: the same chain, the same bits.  Staging, prefetch and
// padding are the other form's (dqn_fetch / dqn_commit).
template <typename XT>
__global__ void __launch_bounds__(256) evg_dqn_qnet_rows16_kernel(DqnArgs a) {
    __shared__ float w1s[DQ_C * DQ_W1S];
    __shared__ float w2s[16 * DQ_OT * DQ_W2S];
    __shared__ float b1s[DQ_C];
    __shared__ float tile[16 * DQ_HS];                 // the workgroup's hidden tile of the chunk, [16][50]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1;
    const int chunks = (H1 + DQ_C - 1) / DQ_C;
    const long long R = a.rows;
    const long long passes = (R + 15) >> 4;
    const XT* __restrict__ xin = static_cast<const XT*>(a.x) + a.x_offset;
    // this wavefront's output tiles: {w, w + 4} and, for wavefront 3, tile 8 (NT: how many)
    const int NT = wave == 3 ? 3 : 2;
    int ot[3];
    ot[0] = wave; ot[1] = wave + 4; ot[2] = 8;
    float b2v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) b2v[i] = 16 * ot[i] + col < DQ_OUT ? a.b2[16 * ot[i] + col] : 0.0f;

    for (long long pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const long long ra = pass * 16 + col;
        const bool va = ra < R;
        float xa[DQ_KX];
        if (wave < DQ_CT) {                            // layer 1's wavefronts: the A fragments of x (clamped row and column: inside the buffer)
            const XT* x = xin + (va ? ra : R - 1) * a.x_stride;
#pragma unroll
            for (int s = 0; s < DQ_KX; ++s) {
                const int k = 4 * s + kq;
                const float v = (float)x[4 * s + 3 < DQ_IN ? k : min(k, DQ_IN - 1)];
                xa[s] = (va && (4 * s + 3 < DQ_IN || k < DQ_IN)) ? v : 0.0f;
            }
        } else {
#pragma unroll
            for (int s = 0; s < DQ_KX; ++s) xa[s] = 0.0f;
        }
        __builtin_amdgcn_sched_barrier(0);
        DqnStage st;
        dqn_fetch(st, a, 0, tid);
        qn_f4 acc2[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) acc2[i] = qn_f4{b2v[i], b2v[i], b2v[i], b2v[i]};

        int c = 0;                                     // (h1 >= 1: at least one chunk)
#pragma unroll 1
        do {
            const int c0 = c * DQ_C;
            __syncthreads();                           // every wavefront is done with the chunk and the tile that LDS holds
            dqn_commit(st, c0, H1, w1s, w2s, b1s, tid);
            __syncthreads();
            if (c + 1 < chunks) dqn_fetch(st, a, c0 + DQ_C, tid);
            __builtin_amdgcn_sched_barrier(0);
            if (wave < DQ_CT) {                        // layer 1: column tile `wave` of the chunk
                const float b = b1s[16 * wave + col];
                qn_f4 acc1 = qn_f4{b, b, b, b};
#pragma unroll
                for (int s = 0; s < DQ_KX; ++s) acc1 = qn_mfma(xa[s], w1s[(16 * wave + col) * DQ_W1S + 4 * s + kq], acc1);
                const bool unit = c0 + 16 * wave + col < H1;       // a unit >= h1 is an exact zero whatever its accumulator holds
#pragma unroll
                for (int r = 0; r < 4; ++r) tile[(row0 + r) * DQ_HS + 16 * wave + col] = unit ? qn_relu(acc1[r]) : 0.0f;
            }
            __syncthreads();                           // the tile is whole
#pragma unroll
            for (int s = 0; s < DQ_KC; ++s) {          // layer 2 continued with the chunk's 48 k on this wavefront's output tiles
                const float h = tile[col * DQ_HS + 4 * s + kq];
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < NT) acc2[i] = qn_mfma(h, w2s[(16 * ot[i] + col) * DQ_W2S + 4 * s + kq], acc2[i]);
            }
        } while (++c < chunks);

#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = pass * 16 + row0 + r;
            if (row < R)
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < NT && 16 * ot[i] + col < DQ_OUT) a.out[row * DQ_OUT + 16 * ot[i] + col] = a.final_relu ? qn_relu(acc2[i][r]) : acc2[i][r];
        }
    }
}

template <typename XT>
static int launch_dqn_qnet_typed(const DqnArgs& a, hipStream_t s) {
    if (a.rows <= EVG_DQN_TINY_ROWS) {
        const long long passes = (a.rows + 15) / 16;               // <= 256 = EVG_DQN_MAX_BLOCKS
        hipLaunchKernelGGL((evg_dqn_qnet_rows16_kernel<XT>), dim3((unsigned)passes), dim3(256), 0, s, a);
    } else if (a.rows <= EVG_DQN_SMALL_ROWS) {
        const long long passes = (a.rows + 63) / 64;               // <= 256 = EVG_DQN_MAX_BLOCKS
        hipLaunchKernelGGL((evg_dqn_qnet_kernel<XT, 1>), dim3((unsigned)passes), dim3(256), 0, s, a);
    } else {
        long long blocks = (a.rows + 255) / 256;
        if (blocks > EVG_DQN_MAX_BLOCKS) blocks = EVG_DQN_MAX_BLOCKS;
        hipLaunchKernelGGL((evg_dqn_qnet_kernel<XT, 4>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

int launch_dqn_qnet(const evg_dqn_net& net, long long rows, const void* x, int obs_dtype, long long x_stride, long long x_offset, float* q_out,
                    void* stream) {
    static_assert(EVG_DQN_SMALL_ROWS / 64 <= EVG_DQN_MAX_BLOCKS && EVG_DQN_TINY_ROWS / 16 <= EVG_DQN_MAX_BLOCKS, "the small forms' grids are under the cap");
    const DqnArgs a{net.w1, net.b1, net.w2, net.b2, net.h1, net.final_relu, rows, x, x_stride, x_offset, q_out};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (obs_dtype) {
        case EVG_OBS_F32: return launch_dqn_qnet_typed<float>(a, s);
        case EVG_OBS_F64: return launch_dqn_qnet_typed<double>(a, s);
        case EVG_OBS_I16: return launch_dqn_qnet_typed<int16_t>(a, s);
        default: return -1;
    }
}

// ---------------------------------------------------------------------------------------------
// network output -> orders: DQNAgent.filter_actions / epsilon_greedy (dqn_decode.inc).  One env per lane, 64 envs per workgroup: the walk is sequential
// by nature (132 values x up to 7 slots).  The wavefront copies its envs' 64 x 528 contiguous bytes to LDS with coalesced 16-byte loads, transposed to
// [value][env] (stride 65: a lane's reads fall into its own bank), and every lane then walks its env -- the node loop rolled, the twelve groups of a
// node and the seven slots unrolled, so the slots are registers with constant indices.  EXPLORE: the lane first draws its env's coin and random rows
// (two Philox blocks); the turn that keys them is the handle's, as in evg_minimized_actions_kernel.
// ---------------------------------------------------------------------------------------------
constexpr int DQ_QS = 65;                              // row stride of the transposed Q block in LDS

template <bool EXPLORE>
__global__ void __launch_bounds__(64) evg_dqn_actions_kernel(int N, const uint32_t* __restrict__ envw, const float* __restrict__ q, int2* __restrict__ actions,
                                                             ExploreArgs X) {
    __shared__ float qt[(DQ_OUT + 4) * DQ_QS];         // (the last four rows: where the lanes past the workgroup's last value store)
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const int live = min(64, N - e0);                  // envs of this workgroup
    const float4* src = reinterpret_cast<const float4*>(q + (size_t)e0 * DQ_OUT);
#pragma unroll
    for (int i = 0; i < DQ_OUT / 4; ++i) {
        // float4 f of the block: values 4 f .. 4 f + 3 of env f / 33.  A lane past the last value loads the last one again and stores it aside:
        // an address chosen ahead of the load, not a lane mask kept across it
        const int f = lane + 64 * i, lim = live * (DQ_OUT / 4);
        const float4 t = src[min(f, lim - 1)];
        const int env = f / (DQ_OUT / 4), k = 4 * (f - (DQ_OUT / 4) * env);
        const int at = f < lim ? k * DQ_QS + env : DQ_OUT * DQ_QS;
        qt[at] = t.x; qt[at + DQ_QS] = t.y; qt[at + 2 * DQ_QS] = t.z; qt[at + 3 * DQ_QS] = t.w;
    }
    qn_wave_sync();
    if (e >= N) return;
    uint2 d = make_uint2(0u, 0u);
    if constexpr (EXPLORE) {
        const int turn = (int)(envw[e] & 0xFFu);
        const uint32_t env_id = X.env_id_base + (uint32_t)e, episode = X.episode[e];
        const uint4 b0 = rng_block(X.seed_lo, X.seed_hi, env_id, episode, RNG_EXPLORE, 0u, turn, 0, X.seat, 0);
        const uint4 b1 = rng_block(X.seed_lo, X.seed_hi, env_id, episode, RNG_EXPLORE, 1u, turn, 0, X.seat, 0);
        d = dqn_explore_words(b0, b1, X.eps_env ? X.eps_env[e] : X.eps);
    }
    if (X.explored) X.explored[e] = (uint8_t)(d.x >> 31);
    DqnSlots s;
#pragma unroll
    for (int i = 0; i < NA; ++i) { s.best[i] = 0.0f; s.unit[i] = 0; s.node[i] = 0; }
    if (!(d.x >> 31)) {
#pragma unroll 1
        for (int node = 0; node < NN; ++node) {        // node outermost, then group, as the reference walks them (:179-181)
            float v[NG];
#pragma unroll
            for (int group = 0; group < NG; ++group) v[group] = qt[(group * NN + node) * DQ_QS + lane];
#pragma unroll
            for (int group = 0; group < NG; ++group) dqn_filter_step(s, v[group], group, node);
        }
    }
    int2* rows = actions + (size_t)e * NA;
#pragma unroll
    for (int i = 0; i < NA; ++i)                       // the random branch (:156-157), or the slots
        rows[i] = (d.x >> 31) ? make_int2((int)((d.y >> (4 * i)) & 15u), (int)((d.x >> (4 * i)) & 15u)) : make_int2(s.unit[i], s.node[i]);
}

int launch_dqn_actions(const DevState& S, const float* q, int32_t* actions, void* stream, const SmartExplore* ex, uint8_t* explored) {
    const dim3 grid((unsigned)((S.N + 63) / 64)), block(64);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int2* a = reinterpret_cast<int2*>(actions);
    ExploreArgs X{};
    X.explored = explored;
    if (ex) {
        X = ExploreArgs{S.seed_lo, S.seed_hi, S.env_id_base, S.episode, ex->seat, ex->eps, ex->eps_env, explored};
        hipLaunchKernelGGL(evg_dqn_actions_kernel<true>, grid, block, 0, s, S.N, S.env, q, a, X);
    } else {
        hipLaunchKernelGGL(evg_dqn_actions_kernel<false>, grid, block, 0, s, S.N, S.env, q, a, X);
    }
    return (int)hipGetLastError();
}
