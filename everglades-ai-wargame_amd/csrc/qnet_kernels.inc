// qnet_kernels.inc -- the Smart_State Q network's forward pass (include/evg.h, evg_smart_qnet): agents/Smart_State/QNetwork.py, inference only.
// Included by evg_kernels.hip (namespace evg).
//
//   evg_qnet_kernel<EXPANDED>   256 threads = 4 wavefronts; a wavefront owns 16 rows at a time (16 envs of one seat and one swarm index in the compact
//                               layouts, 16 rows of x in the expanded one) and runs all three layers on them with v_mfma_f32_16x16x4_f32
//
// Numerics.  v_mfma_f32_16x16x4_f32 computes D[i][j] = fma(A[i][3] B[3][j], fma(A[i][2] B[2][j], fma(A[i][1] B[1][j], fma(A[i][0] B[0][j], C[i][j]))))
// exactly (one rounding per product, k ascending), so a sequence of them over k-steps 0, 1, 2, ... with C = the bias IS the chain of the contract.
// The operands are always taken in natural k order (the hidden tiles go through LDS, never accumulator-as-operand), and every padded k position has a
// zero weight and a zero input, which leaves the chain unchanged.  The zero input is enforced, not incidental: the ReLU is torch's (x < 0 ? 0 : x, a NaN
// stays a NaN, on the hidden layers and on the output), so a padded hidden unit -- whose accumulator is 0 + sum of x * 0, NaN for an Inf or NaN x -- is
// an exact zero in the tile (zeroed once, never stored to: qn_store_col); otherwise NaN * 0 would poison every output of a row that has one non-finite input.  The compact layouts run the chain prefix b1 + shared[0..33] once per 16 envs and
// continue it per swarm with swarm[s][0..12] (W1 columns 34..46), then add W1[j][47 + s] on the VALU: the one-hot term.
//
// Lane maps (16x16x4 f32): A lane l = X[row l & 15][k l >> 4], B lane l = W[column l & 15][k l >> 4], C/D lane l register r = [row 4 (l >> 4) + r]
// [column l & 15].  The weights live in registers as B fragments (staged through LDS once per workgroup), the rows' inputs are read as A fragments
// straight from HBM, the hidden tiles are written to a per-wavefront LDS tile in the D layout and read back in the A layout.

constexpr int QN_IN = 59, QN_OUT = 5, QN_H = 64;       // input width, output width, the largest hidden size
constexpr int QN_WAVES = 4;                            // wavefronts per workgroup
constexpr int QN_HS = 68;                              // row stride of a hidden tile in LDS (68 = 4 mod 64: the A-layout read is conflict-free; the 4 spare columns take the padded units)
constexpr int QN_W1S = 61, QN_W2S = 65, QN_W3S = 65;   // row strides of the staged weights (odd: the B-fragment reads spread over the banks)
constexpr int QN_STAGE = QN_H * QN_W1S + QN_H * QN_W2S + 16 * QN_W3S;   // staged weights (floats)
constexpr int QN_WAVE_LDS = 2 * 16 * QN_HS + 16 * 60;                    // per wavefront: two hidden tiles and the 16 x 60 Q tile
constexpr int QN_UNION = QN_STAGE > QN_WAVES * QN_WAVE_LDS ? QN_STAGE : QN_WAVES * QN_WAVE_LDS;
constexpr int QN_W1PS = 37;                             // row stride of the staged shared columns W1[:, 0..35] (the compact prefix)
constexpr int QN_FIXED = 64 + 64 + 16 + 12 * 64 + QN_H * QN_W1PS;   // b1, b2, b3, the one-hot columns W1[:, 47 + s], W1[:, 0..35]

typedef float qn_f4 __attribute__((ext_vector_type(4)));

struct QnetSet {
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* w3;
    const float* b3;
};

struct QnetArgs {
    QnetSet set[2];
    int h1, h2, final_relu, num_seats;     // num_seats: the S of the compact layouts (1 or 2); 1 for the expanded one
    long long rows;
    const float* in0;
    const float* in1;
    float* out;
};

__device__ __forceinline__ qn_f4 qn_mfma(float a, float b, qn_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ void qn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// torch.relu: a NaN stays a NaN (fmaxf would drop it); the sign of a zero result is not part of the contract.  IEEE 754-2019 maximum, which gfx950 has
// as one instruction (v_maximum3_f32), so the ReLU costs what fmaxf cost
__device__ __forceinline__ float qn_relu(float x) { return __builtin_elementwise_maximum(x, 0.0f); }

// The column of a hidden tile that unit 16 t + col of a layer of hn units is stored to: its own -- or, for a padded unit (>= hn), one of the row's four
// spare columns (the row stride is 64 + 4), which nothing reads.  A padded unit's accumulator is 0 + sum of x * 0, a NaN as soon as an x is Inf or NaN,
// which the next layer's zero weight would not take out (NaN * 0); stored aside, it leaves the padded columns with the exact zeros that qn_zero_tile
// wrote once, before the wavefront's first group.  Lane-constant, computed before the loop over the groups: the stores stay unconditional.
__device__ __forceinline__ int qn_store_col(int t, int col, int hn, int width) { return 16 * t + col < hn ? 16 * t + col : width + (col & 3); }

// acc (D layout) -> relu -> hidden tile in LDS, tile t to column cols[t] (qn_store_col)
__device__ __forceinline__ void qn_store_hidden(float* __restrict__ tile, const qn_f4 (&acc)[4], const int (&cols)[4], int lane) {
    const int row0 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(row0 + r) * QN_HS + cols[t]] = qn_relu(acc[t][r]);
}

// a wavefront's n floats of LDS <- exact zeros (the padded columns of its hidden tiles are never written again)
__device__ __forceinline__ void qn_zero_tile(float* __restrict__ tile, int n, int lane) {
    for (int i = lane; i < n; i += 64) tile[i] = 0.0f;
}

// Layers 2 and 3 of 16 rows whose first hidden layer (after the ReLU) is in tile h1t: returns the Q tile (D layout; columns 0..4 are Q)
__device__ __forceinline__ qn_f4 qn_layers23(const float* __restrict__ h1t, float* __restrict__ h2t, const float (&w2f)[16][4], const float (&w3f)[16],
                                            const float (&b2v)[4], float b3v, int n2, const int (&cols2)[4], int final_relu, int lane) {
    const int arow = (lane & 15) * QN_HS + (lane >> 4);
    qn_f4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = qn_f4{b2v[t], b2v[t], b2v[t], b2v[t]};
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        if (st < n2) {
            const float a = h1t[arow + 4 * st];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = qn_mfma(a, w2f[st][t], acc[t]);
        }
    }
    qn_store_hidden(h2t, acc, cols2, lane);
    qn_wave_sync();
    qn_f4 q = qn_f4{b3v, b3v, b3v, b3v};
#pragma unroll
    for (int st = 0; st < 16; ++st) q = qn_mfma(h2t[arow + 4 * st], w3f[st], q);   // (k >= h2: zero weight, zero input)
    if (final_relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = qn_relu(q[r]);
    return q;
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_qnet_kernel(QnetArgs a) {
    __shared__ float fixed[QN_FIXED];
    __shared__ __attribute__((aligned(16))) float lds[QN_UNION];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = blockIdx.y;
    const QnetSet W = a.set[seat];
    const int H1 = a.h1, H2 = a.h2, S = a.num_seats;

    // ---- stage the set's weights in LDS, zero-padded to 64 (and 16) rows and to the fragment widths
    float* w1s = lds;
    float* w2s = w1s + QN_H * QN_W1S;
    float* w3s = w2s + QN_H * QN_W2S;
    for (int i = tid; i < QN_H * 60; i += 64 * QN_WAVES) {
        const int j = i / 60, k = i - 60 * j;
        w1s[j * QN_W1S + k] = (j < H1 && k < QN_IN) ? W.w1[j * QN_IN + k] : 0.0f;
    }
    for (int i = tid; i < QN_H * QN_H; i += 64 * QN_WAVES) {
        const int j = i >> 6, k = i & 63;
        w2s[j * QN_W2S + k] = (j < H2 && k < H1) ? W.w2[j * H1 + k] : 0.0f;
    }
    for (int i = tid; i < 16 * QN_H; i += 64 * QN_WAVES) {
        const int j = i >> 6, k = i & 63;
        w3s[j * QN_W3S + k] = (j < QN_OUT && k < H2) ? W.w3[j * H2 + k] : 0.0f;
    }
    for (int i = tid; i < QN_FIXED; i += 64 * QN_WAVES) {
        float v = 0.0f;
        if (i < 64) v = i < H1 ? W.b1[i] : 0.0f;
        else if (i < 128) v = i - 64 < H2 ? W.b2[i - 64] : 0.0f;
        else if (i < 144) v = i - 128 < QN_OUT ? W.b3[i - 128] : 0.0f;
        else if (i < 912) {
            const int s = (i - 144) >> 6, j = (i - 144) & 63;
            v = j < H1 ? W.w1[j * QN_IN + 47 + s] : 0.0f;
        } else {
            const int j = (i - 912) / QN_W1PS, k = (i - 912) - QN_W1PS * j;
            v = (j < H1 && k < 34) ? W.w1[j * QN_IN + k] : 0.0f;
        }
        fixed[i] = v;
    }
    __syncthreads();

    // ---- this lane's B fragments: lane l holds W[16 t + (l & 15)][4 st + (l >> 4)]
    const int col = lane & 15, kq = lane >> 4;
    // (the compact prefix runs once per 16 envs: its 36 fragments are read from LDS there, not kept in registers)
    float w1f[EXPANDED ? 15 : 1][4], w1x[EXPANDED ? 1 : 4][4], w2f[16][4], w3f[16], b1v[4], b2v[4];
    if (EXPANDED)
#pragma unroll
        for (int st = 0; st < 15; ++st)
#pragma unroll
            for (int t = 0; t < 4; ++t) w1f[st][t] = w1s[(16 * t + col) * QN_W1S + 4 * st + kq];
    if (!EXPANDED)
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = 4 * st + kq;               // swarm feature k -> W1 column 34 + k
                w1x[st][t] = k < 13 ? w1s[(16 * t + col) * QN_W1S + 34 + k] : 0.0f;
            }
#pragma unroll
    for (int st = 0; st < 16; ++st) {
#pragma unroll
        for (int t = 0; t < 4; ++t) w2f[st][t] = w2s[(16 * t + col) * QN_W2S + 4 * st + kq];
        w3f[st] = w3s[col * QN_W3S + 4 * st + kq];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        b1v[t] = fixed[16 * t + col];
        b2v[t] = fixed[64 + 16 * t + col];
    }
    const float b3v = fixed[128 + col];
    __syncthreads();                                  // the staging area becomes the wavefronts' tiles

    float* h1t = lds + wave * QN_WAVE_LDS;
    float* h2t = h1t + 16 * QN_HS;
    float* qt = h2t + 16 * QN_HS;
    int cols1[4], cols2[4];                           // where this lane's units of the two hidden layers are stored
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        cols1[t] = qn_store_col(t, col, H1, QN_H);
        cols2[t] = qn_store_col(t, col, H2, QN_H);
    }
    qn_zero_tile(h1t, 2 * 16 * QN_HS, lane);          // both hidden tiles: what was staged there is gone, the padded columns are zeros from here on
    qn_wave_sync();
    const int n2 = (H1 + 3) >> 2;                     // layer-2 k-steps (layer 3 always runs 16: its padded k have zero weights and inputs)
    const int row0 = 4 * kq;
    const long long R = a.rows;
    const long long groups = (R + 15) >> 4;

    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;                // this lane's A row
        const bool va = ra < R;
        if (EXPANDED) {
            const float* x = a.in0 + ra * QN_IN;
            float xa[15];
#pragma unroll
            for (int st = 0; st < 15; ++st) {
                const int k = 4 * st + kq;
                xa[st] = (va && k < QN_IN) ? x[k] : 0.0f;
            }
            qn_f4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = qn_f4{b1v[t], b1v[t], b1v[t], b1v[t]};
#pragma unroll
            for (int st = 0; st < 15; ++st)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = qn_mfma(xa[st], w1f[st][t], acc[t]);
            qn_store_hidden(h1t, acc, cols1, lane);
            qn_wave_sync();
            const qn_f4 q = qn_layers23(h1t, h2t, w2f, w3f, b2v, b3v, n2, cols2, a.final_relu, lane);
            if (col < QN_OUT)
#pragma unroll
                for (int r = 0; r < 4; ++r) qt[(row0 + r) * QN_OUT + col] = q[r];
            qn_wave_sync();
            const long long base = r0 * QN_OUT, end = R * QN_OUT;
            for (int i = lane; i < 16 * QN_OUT; i += 64)
                if (base + i < end) a.out[base + i] = qt[i];
        } else {
            const long long vr = ra * S + seat;      // the row of (env, seat) in [R][S][...]
            const float* sh = a.in0 + vr * 34;
            const float* sw = a.in1 + vr * (12 * 13);
            qn_f4 pre[4];                             // b1 + the 34 shared terms, once per env
#pragma unroll
            for (int t = 0; t < 4; ++t) pre[t] = qn_f4{b1v[t], b1v[t], b1v[t], b1v[t]};
#pragma unroll
            for (int st = 0; st < 9; ++st) {
                const int k = 4 * st + kq;
                const float x = (va && k < 34) ? sh[k] : 0.0f;
#pragma unroll
                for (int t = 0; t < 4; ++t) pre[t] = qn_mfma(x, fixed[912 + (16 * t + col) * QN_W1PS + 4 * st + kq], pre[t]);
            }
            float xs[4];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int k = 4 * st + kq;
                xs[st] = (va && k < 13) ? sw[k] : 0.0f;
            }
#pragma unroll 1
            for (int s = 0; s < 12; ++s) {
                qn_f4 acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = pre[t];
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = qn_mfma(xs[st], w1x[st][t], acc[t]);
                if (s + 1 < 12)                       // the next swarm's inputs, in flight during this swarm's layers 2 and 3
#pragma unroll
                    for (int st = 0; st < 4; ++st) {
                        const int k = 4 * st + kq;
                        xs[st] = (va && k < 13) ? sw[(s + 1) * 13 + k] : 0.0f;
                    }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float oh = fixed[144 + s * 64 + 16 * t + col];   // the one-hot term at position 47 + s
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t][r] = acc[t][r] + oh;
                }
                qn_store_hidden(h1t, acc, cols1, lane);
                qn_wave_sync();
                const qn_f4 q = qn_layers23(h1t, h2t, w2f, w3f, b2v, b3v, n2, cols2, a.final_relu, lane);
                if (col < QN_OUT)
#pragma unroll
                    for (int r = 0; r < 4; ++r) qt[(row0 + r) * 60 + s * QN_OUT + col] = q[r];
            }
            qn_wave_sync();
            // 16 rows x 60 floats: 15 float4 per row, rows (env, seat) at [r0 + i][seat] of [R][S][12][5]
            for (int i = lane; i < 16 * 15; i += 64) {
                const int row = i / 15, c = i - 15 * row;
                if (r0 + row < R)
                    reinterpret_cast<float4*>(a.out + ((r0 + row) * S + seat) * 60)[c] = reinterpret_cast<const float4*>(qt + row * 60)[c];
            }
        }
        qn_wave_sync();                               // the tiles are rewritten by the next group
    }
}

int launch_smart_qnet(const evg_qnet& net, int layout, long long rows, const float* in0, const float* in1, float* q_out, int num_cu, void* stream) {
    QnetArgs a;
    for (int p = 0; p < 2; ++p) {
        const int q = p < net.num_sets ? p : 0;
        a.set[p] = QnetSet{net.w1[q], net.b1[q], net.w2[q], net.b2[q], net.w3[q], net.b3[q]};
    }
    a.h1 = net.h1;
    a.h2 = net.h2;
    a.final_relu = net.final_relu;
    a.num_seats = layout == EVG_QNET_COMPACT_SEATS ? 2 : 1;
    a.rows = rows;
    a.in0 = in0;
    a.in1 = in1;
    a.out = q_out;
    // persistent-style grid: two workgroups per CU are resident (the weight registers allow 2 wavefronts per SIMD); each wavefront loops over its groups
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_qnet_kernel<true>, dim3((unsigned)blocks, 1), dim3(64 * QN_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(evg_qnet_kernel<false>, dim3((unsigned)blocks, (unsigned)a.num_seats), dim3(64 * QN_WAVES), 0, s, a);
    return (int)hipGetLastError();
}
