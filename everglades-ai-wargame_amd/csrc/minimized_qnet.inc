// minimized_qnet.inc -- the Minimized agents' Q network's forward pass (include/evg.h, evg_minimized_qnet): agents/Minimized/QNetwork.py, inference only:
// relu(fc2(relu(fc1(x)))), 59 -> h1 -> 11 with h1 in 1..128 (80 by default, carried in the agents' pickles).  Included by evg_kernels.hip (namespace evg),
// after qnet_kernels.inc, whose helpers (qn_f4, qn_mfma, qn_wave_sync) and numeric contract it shares:
//
//   evg_mini_qnet_kernel<EXPANDED>   256 threads = 4 wavefronts; a wavefront owns 16 rows at a time (16 envs of one seat in the compact layouts, 16 rows of
//                                    x in the expanded one) and runs both layers on them with v_mfma_f32_16x16x4_f32
//
// Numerics: as qnet_kernels.inc -- a sequence of 16x16x4 MFMAs over k-steps 0, 1, 2, ... with C = the bias IS the chain acc = b[j], fmaf(W[j][k], x[k], acc)
// for k ascending; operands in natural k order, padded k positions with zero weight and zero input; the compact layouts run the 34-term shared prefix once
// per 16 envs and add the one-hot term W1[j][47 + s] on the VALU.  The ReLU is torch's (a NaN stays a NaN, hidden layer and output), and the padded
// hidden units inside the last tile (index >= h1) are exact zeros whatever their accumulator holds (0 + sum of x * 0 is NaN for a non-finite x): zeroed once, never stored to.
//
// Hidden up to 128 is up to 8 column tiles of 16; the 11 outputs are one tile.  Tiles beyond the network's h1 are skipped (wave-uniform branches), so a
// network of 80 runs 5.  Registers hold what every group of rows reuses and fits: the 13 swarm columns of W1 (compact; 4 k-steps x 8 tiles), W2 (32 k-steps)
// and the biases.  The layer-1 fragments that do not fit next to them -- all 15 k-steps x 8 tiles of the expanded layout, the 9 x 8 of the compact prefix
// -- are read from LDS at every use, where the whole workgroup shares one zero-padded copy.  The hidden tile goes through a per-wavefront LDS tile (D layout
// in, A layout out); Q leaves the accumulator straight to HBM: a row's 11 values are 44 contiguous bytes.

constexpr int MQ_OUT = 11, MQ_H = 128, MQ_TILES = MQ_H / 16;   // output width, the largest hidden size, its column tiles
constexpr int MQ_HS = 132;                                     // row stride of the hidden tile in LDS (132 = 4 mod 64: the A-layout read is conflict-free; 4 spare columns)
constexpr int MQ_W1S = 61, MQ_W1PS = 37;                       // row strides of the staged W1 (expanded: 60 columns) and of its shared columns (compact: 36)
constexpr int MQ_KX = 15, MQ_KP = 9, MQ_KS = 4, MQ_K2 = MQ_H / 4;   // k-steps: expanded layer 1, compact prefix, swarm columns, layer 2

struct MiniQnetSet {
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
};

struct MiniQnetArgs {
    MiniQnetSet set[2];
    int h1, final_relu, num_seats;     // num_seats: the S of the compact layouts (1 or 2); 1 for the expanded one
    long long rows;
    const float* in0;
    const float* in1;
    float* out;
};

// layer 2 of 16 rows whose hidden layer (after the ReLU) is in tile ht: the Q tile (D layout; columns 0..10 are Q)
// (k runs over the nt column tiles layer 1 wrote: k >= h1 inside the last tile has a zero weight and an exact zero input: qn_store_col)
__device__ __forceinline__ qn_f4 mq_layer2(const float* __restrict__ ht, const float (&w2f)[MQ_K2], float b2v, int nt, int final_relu, int lane) {
    const int arow = (lane & 15) * MQ_HS + (lane >> 4);
    qn_f4 q = qn_f4{b2v, b2v, b2v, b2v};
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t)
        if (t < nt)
#pragma unroll
            for (int st = 4 * t; st < 4 * t + 4; ++st) q = qn_mfma(ht[arow + 4 * st], w2f[st], q);
    if (final_relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = qn_relu(q[r]);
    return q;
}

// acc (D layout) of a column tile -> relu (qn_relu: a NaN stays) -> column c of the hidden tile (qn_store_col: the padded units of the last tile,
// >= h1, go to the row's spare columns 128..131, and theirs keep the exact zeros the tile was filled with before the wavefront's first group)
__device__ __forceinline__ void mq_store_hidden(float* __restrict__ ht, const qn_f4 acc, int c, int lane) {
    const int row0 = 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) ht[(row0 + r) * MQ_HS + c] = qn_relu(acc[r]);
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_mini_qnet_kernel(MiniQnetArgs a) {
    // the workgroup's copy of the layer-1 weights that are read at every use: expanded W1[:, 0..59] (stride 61); compact W1[:, 0..35] (stride 37), then
    // the one-hot columns W1[:, 47 + s] as [12][128]
    constexpr int WLDS = EXPANDED ? MQ_H * MQ_W1S : MQ_H * MQ_W1PS + 12 * MQ_H;
    __shared__ float wl[WLDS];
    __shared__ float tiles[QN_WAVES][16 * MQ_HS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = blockIdx.y;
    const MiniQnetSet W = a.set[seat];
    const int H1 = a.h1, S = a.num_seats;
    const int nt = (H1 + 15) >> 4;                     // column tiles of the hidden layer

    if (EXPANDED) {
        for (int i = tid; i < MQ_H * 60; i += 64 * QN_WAVES) {
            const int j = i / 60, k = i - 60 * j;
            wl[j * MQ_W1S + k] = (j < H1 && k < QN_IN) ? W.w1[j * QN_IN + k] : 0.0f;
        }
    } else {
        for (int i = tid; i < MQ_H * 36; i += 64 * QN_WAVES) {
            const int j = i / 36, k = i - 36 * j;
            wl[j * MQ_W1PS + k] = (j < H1 && k < 34) ? W.w1[j * QN_IN + k] : 0.0f;
        }
        for (int i = tid; i < 12 * MQ_H; i += 64 * QN_WAVES) {
            const int s = i >> 7, j = i & (MQ_H - 1);
            wl[MQ_H * MQ_W1PS + i] = j < H1 ? W.w1[j * QN_IN + 47 + s] : 0.0f;
        }
    }

    // ---- this lane's B fragments and biases, straight from the caller's tensors: lane l holds W[16 t + (l & 15)][4 st + (l >> 4)]
    const int col = lane & 15, kq = lane >> 4;
    float w1x[EXPANDED ? 1 : MQ_KS][MQ_TILES], w2f[MQ_K2], b1v[MQ_TILES];
    if (!EXPANDED)
#pragma unroll
        for (int st = 0; st < MQ_KS; ++st)
#pragma unroll
            for (int t = 0; t < MQ_TILES; ++t) {
                const int j = 16 * t + col, k = 4 * st + kq;            // swarm feature k -> W1 column 34 + k
                w1x[st][t] = (j < H1 && k < 13) ? W.w1[j * QN_IN + 34 + k] : 0.0f;
            }
#pragma unroll
    for (int st = 0; st < MQ_K2; ++st) {
        const int k = 4 * st + kq;
        w2f[st] = (col < MQ_OUT && k < H1) ? W.w2[col * H1 + k] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t) b1v[t] = 16 * t + col < H1 ? W.b1[16 * t + col] : 0.0f;
    const float b2v = col < MQ_OUT ? W.b2[col] : 0.0f;
    float* ht = tiles[wave];
    int cols[MQ_TILES];                               // where this lane's units of the hidden layer are stored
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t) cols[t] = qn_store_col(t, col, H1, MQ_H);
    qn_zero_tile(ht, 16 * MQ_HS, lane);               // the padded columns of the last tile are zeros from here on
    __syncthreads();

    const int row0 = 4 * kq;
    const long long R = a.rows;
    const long long groups = (R + 15) >> 4;

    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;                // this lane's A row
        const bool va = ra < R;
        // (the lane's k offset, opaque once per group: the masks of the guarded input loads below are then recomputed next to their loads -- one compare
        // each -- instead of being kept across the loop as one SGPR pair per k-step, which spilled)
        int kv = kq;
        asm volatile("" : "+v"(kv));
        if (EXPANDED) {
            const float* x = a.in0 + ra * QN_IN;
            float xa[MQ_KX];
#pragma unroll
            for (int st = 0; st < MQ_KX; ++st) {
                const int k = 4 * st + kv;
                xa[st] = (va && k < QN_IN) ? x[k] : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < MQ_TILES; ++t)
                if (t < nt) {
                    qn_f4 acc = qn_f4{b1v[t], b1v[t], b1v[t], b1v[t]};
#pragma unroll
                    for (int st = 0; st < MQ_KX; ++st) acc = qn_mfma(xa[st], wl[(16 * t + col) * MQ_W1S + 4 * st + kq], acc);
                    mq_store_hidden(ht, acc, cols[t], lane);
                }
            qn_wave_sync();
            const qn_f4 q = mq_layer2(ht, w2f, b2v, nt, a.final_relu, lane);
            if (col < MQ_OUT)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (r0 + row0 + r < R) a.out[(r0 + row0 + r) * MQ_OUT + col] = q[r];
        } else {
            const long long vr = ra * S + seat;      // the row of (env, seat) in [R][S][...]
            const float* sh = a.in0 + vr * 34;
            const float* sw = a.in1 + vr * (12 * 13);
            qn_f4 pre[MQ_TILES];                      // b1 + the 34 shared terms, once per env
            {
                float xp[MQ_KP];
#pragma unroll
                for (int st = 0; st < MQ_KP; ++st) {
                    const int k = 4 * st + kv;
                    xp[st] = (va && k < 34) ? sh[k] : 0.0f;
                }
#pragma unroll
                for (int t = 0; t < MQ_TILES; ++t) {
                    pre[t] = qn_f4{b1v[t], b1v[t], b1v[t], b1v[t]};
                    if (t < nt)
#pragma unroll
                        for (int st = 0; st < MQ_KP; ++st) pre[t] = qn_mfma(xp[st], wl[(16 * t + col) * MQ_W1PS + 4 * st + kq], pre[t]);
                }
            }
            float xs[MQ_KS];
#pragma unroll
            for (int st = 0; st < MQ_KS; ++st) {
                const int k = 4 * st + kv;
                xs[st] = (va && k < 13) ? sw[k] : 0.0f;
            }
#pragma unroll 1
            for (int s = 0; s < 12; ++s) {
#pragma unroll
                for (int t = 0; t < MQ_TILES; ++t)
                    if (t < nt) {
                        qn_f4 acc = pre[t];
#pragma unroll
                        for (int st = 0; st < MQ_KS; ++st) acc = qn_mfma(xs[st], w1x[st][t], acc);
                        const float oh = wl[MQ_H * MQ_W1PS + s * MQ_H + 16 * t + col];   // the one-hot term at position 47 + s
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[r] = acc[r] + oh;
                        mq_store_hidden(ht, acc, cols[t], lane);
                    }
                if (s + 1 < 12) {                     // the next swarm's inputs, in flight during this swarm's layer 2
                    asm volatile("" : "+v"(kv));
#pragma unroll
                    for (int st = 0; st < MQ_KS; ++st) {
                        const int k = 4 * st + kv;
                        xs[st] = (va && k < 13) ? sw[(s + 1) * 13 + k] : 0.0f;
                    }
                }
                qn_wave_sync();
                const qn_f4 q = mq_layer2(ht, w2f, b2v, nt, a.final_relu, lane);
                // rows (env, seat) at [r0 + i][seat] of [R][S][12][11]
                if (col < MQ_OUT)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r0 + row0 + r < R) a.out[((r0 + row0 + r) * S + seat) * (12 * MQ_OUT) + s * MQ_OUT + col] = q[r];
                qn_wave_sync();                       // the tile is rewritten by the next swarm
            }
        }
        qn_wave_sync();                               // the tile is rewritten by the next group
    }
}

int launch_minimized_qnet(const evg_mini_qnet& net, int layout, long long rows, const float* in0, const float* in1, float* q_out, int num_cu, void* stream) {
    MiniQnetArgs a;
    for (int p = 0; p < 2; ++p) {
        const int q = p < net.num_sets ? p : 0;
        a.set[p] = MiniQnetSet{net.w1[q], net.b1[q], net.w2[q], net.b2[q]};
    }
    a.h1 = net.h1;
    a.final_relu = net.final_relu;
    a.num_seats = layout == EVG_QNET_COMPACT_SEATS ? 2 : 1;
    a.rows = rows;
    a.in0 = in0;
    a.in1 = in1;
    a.out = q_out;
    // persistent-style grid: two workgroups per CU are resident (LDS); each wavefront loops over its groups
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_mini_qnet_kernel<true>, dim3((unsigned)blocks, 1), dim3(64 * QN_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(evg_mini_qnet_kernel<false>, dim3((unsigned)blocks, (unsigned)a.num_seats), dim3(64 * QN_WAVES), 0, s, a);
    return (int)hipGetLastError();
}
