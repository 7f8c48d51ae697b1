// qnet_grad_kernels.inc -- the backward pass of the two Q networks' expanded fp32 forward (include/evg_qnet_grad.h: evg_smart_qnet_backward,
// evg_minimized_qnet_backward): the parameter gradients of optimize_model's policy forward.  Included by evg_kernels.hip (namespace evg) under EVG_GRAD
// (`make grad`, libevg_grad.so), after qnet_kernels.inc and minimized_qnet.inc, whose argument sets, lane maps and layer functions (qn_mfma,
// qn_store_hidden, qn_layers23, mq_store_hidden, mq_layer2) it uses: the forward chain of layers 2 and 3 is the forward's own code, and layer 1 is its
// fifteen k-steps with the bias as C.  The forward's kernel bodies (qnet_body.inc, minimized_qnet_body.inc) are not included: their LDS is a union of the
// staged weights and the wavefronts' tiles, and the backward needs W2 and W3 in LDS for as long as it runs.
//
//   evg_qnet_grad_kernel        59 -> h1 -> h2 -> 5   256 threads = 4 wavefronts, one wavefront per SIMD (up to 512 registers each)
//   evg_mini_qnet_grad_kernel   59 -> h1 -> 11
//   evg_qnet_grad_reduce_kernel the workgroups' partials -> the gradient tensors, in ascending workgroup order, with the optional clamp
//
// A wavefront loops over groups of 16 rows.  For a group it recomputes a1, a2, q (tiles in LDS, q in the D layout), forms the deltas and adds the
// group's outer products into accumulator tiles that live in registers for the whole launch.
//
// Tile maps (v_mfma_f32_16x16x4_f32: A lane l = A[l & 15][l >> 4], B lane l = B[l >> 4][l & 15], D lane l register r = D[4 (l >> 4) + r][l & 15]).
//   outer products   gW[j][i] = sum over rows of d[row][j] a[row][i]: the row index is the MFMA's k.  The contract leaves the order of that sum open,
//                    so k-step st of lane quarter kq is taken to be row 4 kq + st: then register st of a delta tile in the D layout (rows 4 kq + r,
//                    unit l & 15) IS the A fragment of d^T for k-step st, with no transpose; the B fragment is a[4 kq + st][16 t + (l & 15)], read
//                    from the activation tile in LDS (row stride = 4 mod 64: the four quarters fall on disjoint banks), or from memory for x.
//   W^T d            d_prev[row][i] = sum_j d[row][j] W[j][i]: d goes through LDS into the A layout (as the forward's hidden tiles do), W[j][i] is
//                    read from LDS as B[k = j][n = i] (row stride 80 = 16 mod 64: conflict-free).
// The masks are a > 0 on the activation tile itself (Smart_State), or bits kept from the layer-1 accumulators (Minimized, whose one tile is reused for
// d2); a padded unit's activation is the exact zero of the forward's tile, so its mask is 0 and its delta an exact zero (a select, not a product).
//
// End of the launch: the four wavefronts' accumulators go through LDS, are summed in wavefront order, and the sum is the workgroup's partial in the
// caller's workspace (padded shapes: EVG_*_QNET_GRAD_PARTIAL floats).  No atomics anywhere: the order of every sum is a function of the grid alone.

constexpr int QG_W2S = 80;                              // row stride of W2 / W3 in LDS as B[k = unit out][n = unit in]
constexpr int QG_DS = 20;                               // row stride of the d3 tile (20: the A-layout read is conflict-free)
constexpr int QG_WAVE_LDS = 2 * 16 * QN_HS + 16 * QG_DS;   // per wavefront: the two hidden tiles and the d3 tile
constexpr int QG_LDS = 64 * QG_W2S + 8 * QG_W2S + QN_WAVES * QG_WAVE_LDS;
constexpr int QG_CHUNK = 3072;                          // floats of the partial that the four wavefronts sum at a time (48 rows of 64)
constexpr int QG_P = EVG_SMART_QNET_GRAD_PARTIAL, MG_P = EVG_MINI_QNET_GRAD_PARTIAL;
constexpr int MG_CHUNK = 2048;                          // 32 rows of gW1, or all of gW2 [16][128]
static_assert(QN_WAVES * QG_CHUNK <= QG_LDS && 3 * QG_CHUNK + 144 == QG_P, "the Smart_State partial is three chunks and the biases");
static_assert(5 * MG_CHUNK + 144 == MG_P, "the Minimized partial is five chunks and the biases");

struct QnetGradArgs {
    QnetSet W;
    int h1, h2, final_relu;
    long long rows;
    const float* x;
    const float* gq;
    float* partial;
};

__device__ __forceinline__ float qg_sum4(const qn_f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

__global__ void __launch_bounds__(64 * QN_WAVES) evg_qnet_grad_kernel(QnetGradArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[QG_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1, H2 = a.h2;
    const QnetSet W = a.W;
    float* w2b = lds;                                   // W2[j][i] at j * QG_W2S + i, zero-padded to 64 x 64
    float* w3b = w2b + 64 * QG_W2S;                     // W3[o][j] at o * QG_W2S + j, zero-padded to 8 x 64
    float* h1t = w3b + 8 * QG_W2S + wave * QG_WAVE_LDS;
    float* h2t = h1t + 16 * QN_HS;
    float* dt = h2t + 16 * QN_HS;
    for (int i = tid; i < 64 * 64; i += 64 * QN_WAVES) {
        const int j = i >> 6, k = i & 63;
        w2b[j * QG_W2S + k] = (j < H2 && k < H1) ? W.w2[j * H1 + k] : 0.0f;
    }
    for (int i = tid; i < 8 * 64; i += 64 * QN_WAVES) {
        const int o = i >> 6, k = i & 63;
        w3b[o * QG_W2S + k] = (o < QN_OUT && k < H2) ? W.w3[o * H2 + k] : 0.0f;
    }
    // ---- the forward's B fragments, straight from the caller's tensors: lane l holds W[16 t + (l & 15)][4 st + (l >> 4)]
    float w1f[15][4], w2f[16][4], w3f[16], b1v[4], b2v[4];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        const int k = 4 * st + kq;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = 16 * t + col;
            if (st < 15) w1f[st < 15 ? st : 0][t] = (j < H1 && k < QN_IN) ? W.w1[j * QN_IN + k] : 0.0f;
            w2f[st][t] = (j < H2 && k < H1) ? W.w2[j * H1 + k] : 0.0f;
        }
        w3f[st] = (col < QN_OUT && k < H2) ? W.w3[col * H2 + k] : 0.0f;
    }
    int cols1[4], cols2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        b1v[t] = 16 * t + col < H1 ? W.b1[16 * t + col] : 0.0f;
        b2v[t] = 16 * t + col < H2 ? W.b2[16 * t + col] : 0.0f;
        cols1[t] = qn_store_col(t, col, H1, QN_H);
        cols2[t] = qn_store_col(t, col, H2, QN_H);
    }
    const float b3v = col < QN_OUT ? W.b3[col] : 0.0f;
    qn_zero_tile(h1t, QG_WAVE_LDS, lane);             // the padded columns of the hidden tiles are zeros from here on
    __syncthreads();

    // the accumulators, as row blocks of 16 x 64 of the partial: G[0..3] gW1 (units 16 n ..), G[4..7] gW2, G[8] gW3 (outputs 0..15)
    qn_f4 G[9][4];
#pragma unroll
    for (int n = 0; n < 9; ++n)
#pragma unroll
        for (int t = 0; t < 4; ++t) G[n][t] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};
    float gb1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gb2[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gb3 = 0.0f;   // this lane's rows of the bias sums (unit 16 t + col)

    const int n2 = (H1 + 3) >> 2;
    const long long R = a.rows, groups = (R + 15) >> 4;
    const int arow = col * QN_HS + kq;
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;                // this lane's A row of the forward
        const bool va = ra < R;
        const float* x = a.x + ra * QN_IN;
        float xa[15];
#pragma unroll
        for (int st = 0; st < 15; ++st) {
            const int k = 4 * st + kq;
            xa[st] = (va && k < QN_IN) ? x[k] : 0.0f;
        }
        float xb[4][4], gv[4];                        // x as the B fragments of gW1: x[r0 + 4 kq + st][16 t + col]; gq in the D layout
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const long long row = r0 + row0 + st;
#pragma unroll
            for (int t = 0; t < 4; ++t) xb[st][t] = (row < R && 16 * t + col < QN_IN) ? a.x[row * QN_IN + 16 * t + col] : 0.0f;
            gv[st] = (row < R && col < QN_OUT) ? a.gq[row * QN_OUT + col] : 0.0f;
        }
        // ---- forward: the chain of the contract
        qn_f4 q;
        {
            qn_f4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = qn_f4{b1v[t], b1v[t], b1v[t], b1v[t]};
#pragma unroll
            for (int st = 0; st < 15; ++st)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = qn_mfma(xa[st], w1f[st][t], acc[t]);
            qn_store_hidden(h1t, acc, cols1, lane);
            qn_wave_sync();
            q = qn_layers23(h1t, h2t, w2f, w3f, b2v, b3v, n2, cols2, a.final_relu, lane);
        }
        // ---- d3 (D layout: rows 4 kq + r, output col; zero for col >= 5 and for rows past the end), gb3, gW3
        qn_f4 d3;
#pragma unroll
        for (int r = 0; r < 4; ++r) d3[r] = (!a.final_relu || q[r] > 0.0f) ? gv[r] : 0.0f;
        gb3 += qg_sum4(d3);
#pragma unroll
        for (int r = 0; r < 4; ++r) dt[(row0 + r) * QG_DS + col] = d3[r];
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int t = 0; t < 4; ++t) G[8][t] = qn_mfma(d3[st], h2t[(row0 + st) * QN_HS + 16 * t + col], G[8][t]);
        qn_wave_sync();
        // ---- d2 = (d3 . W3) masked by a2 > 0, gb2, gW2
        const float da0 = dt[col * QG_DS + kq], da1 = dt[col * QG_DS + 4 + kq];
        qn_f4 d2[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            d2[t] = qn_mfma(da1, w3b[(4 + kq) * QG_W2S + 16 * t + col], qn_mfma(da0, w3b[kq * QG_W2S + 16 * t + col], qn_f4{0.0f, 0.0f, 0.0f, 0.0f}));
#pragma unroll
            for (int r = 0; r < 4; ++r) d2[t][r] = h2t[(row0 + r) * QN_HS + 16 * t + col] > 0.0f ? d2[t][r] : 0.0f;
            gb2[t] += qg_sum4(d2[t]);
        }
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
                const float b = h1t[(row0 + st) * QN_HS + 16 * ti + col];
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) G[4 + tj][ti] = qn_mfma(d2[tj][st], b, G[4 + tj][ti]);
            }
        qn_wave_sync();                               // a2 has been read: its tile takes d2 (a padded unit's d2 is an exact zero: the padded columns stay zeros)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) h2t[(row0 + r) * QN_HS + 16 * t + col] = d2[t][r];
        qn_wave_sync();
        // ---- d1 = (d2 . W2) masked by a1 > 0, gb1, gW1
        qn_f4 d1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) d1[t] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const float da = h2t[arow + 4 * st];
#pragma unroll
            for (int t = 0; t < 4; ++t) d1[t] = qn_mfma(da, w2b[(4 * st + kq) * QG_W2S + 16 * t + col], d1[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) d1[t][r] = h1t[(row0 + r) * QN_HS + 16 * t + col] > 0.0f ? d1[t][r] : 0.0f;
            gb1[t] += qg_sum4(d1[t]);
        }
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) G[tj][tk] = qn_mfma(d1[tj][st], xb[st][tk], G[tj][tk]);
        qn_wave_sync();                               // the tiles are rewritten by the next group
    }

    // ---- the workgroup's partial: the four wavefronts' accumulators through LDS, summed in wavefront order
    __syncthreads();                                  // (the weights and the tiles are done with)
    float* P = a.partial + (long long)blockIdx.x * QG_P;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int n = 0; n < 3; ++n)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) lds[wave * QG_CHUNK + (16 * n + row0 + r) * 64 + 16 * t + col] = G[3 * c + n][t][r];
        __syncthreads();
        for (int i = tid; i < QG_CHUNK; i += 64 * QN_WAVES)
            P[c * QG_CHUNK + i] = ((lds[i] + lds[QG_CHUNK + i]) + lds[2 * QG_CHUNK + i]) + lds[3 * QG_CHUNK + i];
        __syncthreads();
    }
    // the bias sums: 16 parts (wavefront, lane quarter) of 144, summed in that order
    float* bs = lds + (wave * 4 + kq) * 144;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        bs[16 * t + col] = gb1[t];
        bs[64 + 16 * t + col] = gb2[t];
    }
    bs[128 + col] = gb3;
    __syncthreads();
    if (tid < 144) {
        float s = lds[tid];
        for (int p = 1; p < 16; ++p) s += lds[p * 144 + tid];
        P[3 * QG_CHUNK + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------ Minimized: 59 -> h1 -> 11
struct MiniQnetGradArgs {
    MiniQnetSet W;
    int h1, final_relu;
    long long rows;
    const float* x;
    const float* gq;
    float* partial;
};

__global__ void __launch_bounds__(64 * QN_WAVES) evg_mini_qnet_grad_kernel(MiniQnetGradArgs a) {
    // the workgroup's zero-padded copy of W1[:, 0..59] (stride 61), read at every use as in the forward; the wavefronts' hidden tiles
    __shared__ __attribute__((aligned(16))) float lds[MQ_H * MQ_W1S + QN_WAVES * 16 * MQ_HS];
    static_assert(QN_WAVES * MG_CHUNK <= MQ_H * MQ_W1S + QN_WAVES * 16 * MQ_HS, "the staging of a chunk fits the LDS");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1;
    const int nt = (H1 + 15) >> 4;                     // column tiles of the hidden layer
    const MiniQnetSet W = a.W;
    float* wl = lds;
    float* ht = lds + MQ_H * MQ_W1S + wave * 16 * MQ_HS;
    for (int i = tid; i < MQ_H * 60; i += 64 * QN_WAVES) {
        const int j = i / 60, k = i - 60 * j;
        wl[j * MQ_W1S + k] = (j < H1 && k < QN_IN) ? W.w1[j * QN_IN + k] : 0.0f;
    }
    // W2 twice: the forward's B fragments W2[col][4 st + kq], and for W2^T d2 the fragments B[k = output 4 st + kq][n = unit 16 t + col]
    float w2f[MQ_K2], w2t[3][MQ_TILES], b1v[MQ_TILES];
#pragma unroll
    for (int st = 0; st < MQ_K2; ++st) {
        const int k = 4 * st + kq;
        w2f[st] = (col < MQ_OUT && k < H1) ? W.w2[col * H1 + k] : 0.0f;
    }
    int cols[MQ_TILES];
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t) {
        const int j = 16 * t + col;
#pragma unroll
        for (int st = 0; st < 3; ++st) w2t[st][t] = (4 * st + kq < MQ_OUT && j < H1) ? W.w2[(4 * st + kq) * H1 + j] : 0.0f;
        b1v[t] = j < H1 ? W.b1[j] : 0.0f;
        cols[t] = qn_store_col(t, col, H1, MQ_H);
    }
    const float b2v = col < MQ_OUT ? W.b2[col] : 0.0f;
    qn_zero_tile(ht, 16 * MQ_HS, lane);
    __syncthreads();

    qn_f4 G1[MQ_TILES][4], G2[MQ_TILES];              // gW1 [units 16 t ..][k 16 tk ..], gW2 [outputs 0..15][units 16 t ..]
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t) {
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) G1[t][tk] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};
        G2[t] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    float gb1[MQ_TILES], gb2 = 0.0f;
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t) gb1[t] = 0.0f;

    const long long R = a.rows, groups = (R + 15) >> 4;
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;
        const bool va = ra < R;
        const float* x = a.x + ra * QN_IN;
        float xa[MQ_KX];
#pragma unroll
        for (int st = 0; st < MQ_KX; ++st) {
            const int k = 4 * st + kq;
            xa[st] = (va && k < QN_IN) ? x[k] : 0.0f;
        }
        float xb[4][4], gv[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const long long row = r0 + row0 + st;
#pragma unroll
            for (int t = 0; t < 4; ++t) xb[st][t] = (row < R && 16 * t + col < QN_IN) ? a.x[row * QN_IN + 16 * t + col] : 0.0f;
            gv[st] = (row < R && col < MQ_OUT) ? a.gq[row * MQ_OUT + col] : 0.0f;
        }
        // ---- forward; bit 4 t + r of `active`: a1[4 kq + r][16 t + col] > 0 (a padded unit's accumulator is 0 + sum of x * 0 = 0: not active)
        unsigned active = 0;
#pragma unroll
        for (int t = 0; t < MQ_TILES; ++t)
            if (t < nt) {
                qn_f4 acc = qn_f4{b1v[t], b1v[t], b1v[t], b1v[t]};
#pragma unroll
                for (int st = 0; st < MQ_KX; ++st) acc = qn_mfma(xa[st], wl[(16 * t + col) * MQ_W1S + 4 * st + kq], acc);
                mq_store_hidden(ht, acc, cols[t], lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) active |= (acc[r] > 0.0f && 16 * t + col < H1) ? 1u << (4 * t + r) : 0u;
            }
        qn_wave_sync();
        const qn_f4 q = mq_layer2(ht, w2f, b2v, nt, a.final_relu, lane);
        // ---- d2 (D layout; zero for col >= 11 and for rows past the end), gb2, gW2
        qn_f4 d2;
#pragma unroll
        for (int r = 0; r < 4; ++r) d2[r] = (!a.final_relu || q[r] > 0.0f) ? gv[r] : 0.0f;
        gb2 += qg_sum4(d2);
#pragma unroll
        for (int t = 0; t < MQ_TILES; ++t)
            if (t < nt)
#pragma unroll
                for (int st = 0; st < 4; ++st) G2[t] = qn_mfma(d2[st], ht[(row0 + st) * MQ_HS + 16 * t + col], G2[t]);
        qn_wave_sync();                               // a1 has been read: columns 0..15 of its tile carry d2 into the A layout
#pragma unroll
        for (int r = 0; r < 4; ++r) ht[(row0 + r) * MQ_HS + col] = d2[r];
        qn_wave_sync();
        float da[3];
#pragma unroll
        for (int st = 0; st < 3; ++st) da[st] = ht[col * MQ_HS + 4 * st + kq];
        qn_wave_sync();
#pragma unroll
        for (int r = 0; r < 4; ++r) ht[(row0 + r) * MQ_HS + col] = 0.0f;   // (the next group stores its real units there; a padded column is a zero again)
        // ---- d1 = (d2 . W2) masked by a1 > 0, gb1, gW1
#pragma unroll
        for (int t = 0; t < MQ_TILES; ++t)
            if (t < nt) {
                qn_f4 d1 = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int st = 0; st < 3; ++st) d1 = qn_mfma(da[st], w2t[st][t], d1);
#pragma unroll
                for (int r = 0; r < 4; ++r) d1[r] = (active >> (4 * t + r)) & 1u ? d1[r] : 0.0f;
                gb1[t] += qg_sum4(d1);
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int tk = 0; tk < 4; ++tk) G1[t][tk] = qn_mfma(d1[st], xb[st][tk], G1[t][tk]);
            }
        qn_wave_sync();                               // the tile is rewritten by the next group
    }

    // ---- the workgroup's partial: gW1 [128][64] in four chunks of 32 rows, gW2 [16][128], then the bias sums
    __syncthreads();
    float* P = a.partial + (long long)blockIdx.x * MG_P;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        if (c < 4) {
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                    for (int r = 0; r < 4; ++r) lds[wave * MG_CHUNK + (16 * n + row0 + r) * 64 + 16 * tk + col] = G1[c < 4 ? 2 * c + n : 0][tk][r];
        } else {
#pragma unroll
            for (int t = 0; t < MQ_TILES; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) lds[wave * MG_CHUNK + (row0 + r) * MQ_H + 16 * t + col] = G2[t][r];
        }
        __syncthreads();
        for (int i = tid; i < MG_CHUNK; i += 64 * QN_WAVES)
            P[c * MG_CHUNK + i] = ((lds[i] + lds[MG_CHUNK + i]) + lds[2 * MG_CHUNK + i]) + lds[3 * MG_CHUNK + i];
        __syncthreads();
    }
    float* bs = lds + (wave * 4 + kq) * 144;
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t) bs[16 * t + col] = gb1[t];
    bs[128 + col] = gb2;
    __syncthreads();
    if (tid < 144) {
        float s = lds[tid];
        for (int p = 1; p < 16; ++p) s += lds[p * 144 + tid];
        P[5 * MG_CHUNK + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the reduction
// One thread per element of the gradient tensors (the nn.Linear shapes: nothing outside them is written): the sum of that element over the workgroups'
// partials in ascending workgroup order, the optional clamp, one store.
struct QnetGradSeg {
    float* dst;                                         // [rows][cols], contiguous
    int rows, cols, src, ld;                            // element [j][i] is partial[src + j * ld + i]
};

struct QnetGradReduceArgs {
    QnetGradSeg seg[6];
    int nseg, blocks, stride, total;                    // partials, floats per partial, elements over all segments
    float clamp;
    const float* partial;
};

__global__ void __launch_bounds__(256) evg_qnet_grad_reduce_kernel(QnetGradReduceArgs a) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    int s = 0;
    while (s + 1 < a.nseg && e >= a.seg[s].rows * a.seg[s].cols) {
        e -= a.seg[s].rows * a.seg[s].cols;
        ++s;
    }
    const QnetGradSeg sg = a.seg[s];
    const int j = e / sg.cols, i = e - j * sg.cols;
    const float* __restrict__ p = a.partial + sg.src + j * sg.ld + i;
    float v = 0.0f;
    int b = 0;
    for (; b + 8 <= a.blocks; b += 8) {                 // (eight loads in flight; the additions keep their order)
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(long long)(b + u) * a.stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; b < a.blocks; ++b) v += p[(long long)b * a.stride];
    if (a.clamp > 0.0f) v = fminf(fmaxf(v, -a.clamp), a.clamp);
    sg.dst[e] = v;
}

// workgroups of a backward launch: a function of rows and the device's CU count alone
long long qnet_grad_blocks(long long rows, int num_cu) {
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (cap > EVG_QNET_GRAD_MAX_BLOCKS) cap = EVG_QNET_GRAD_MAX_BLOCKS;
    return blocks < cap ? blocks : cap;
}

static int launch_qnet_grad_reduce(QnetGradReduceArgs& r, hipStream_t s) {
    r.total = 0;
    for (int i = 0; i < r.nseg; ++i) r.total += r.seg[i].rows * r.seg[i].cols;
    hipLaunchKernelGGL(evg_qnet_grad_reduce_kernel, dim3((unsigned)((r.total + 255) / 256)), dim3(256), 0, s, r);
    return (int)hipGetLastError();
}

int launch_smart_qnet_backward(const evg_qnet& net, long long rows, const float* x, const float* gq, const evg_qnet_grads& out, float* workspace,
                               float clamp, int num_cu, void* stream) {
    QnetGradArgs a;
    a.W = QnetSet{net.w1[0], net.b1[0], net.w2[0], net.b2[0], net.w3[0], net.b3[0]};
    a.h1 = net.h1;
    a.h2 = net.h2;
    a.final_relu = net.final_relu;
    a.rows = rows;
    a.x = x;
    a.gq = gq;
    a.partial = workspace;
    const long long blocks = qnet_grad_blocks(rows, num_cu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_qnet_grad_kernel, dim3((unsigned)blocks), dim3(64 * QN_WAVES), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    QnetGradReduceArgs r;
    r.seg[0] = QnetGradSeg{out.w1, net.h1, QN_IN, 0, 64};
    r.seg[1] = QnetGradSeg{out.w2, net.h2, net.h1, 4096, 64};
    r.seg[2] = QnetGradSeg{out.w3, QN_OUT, net.h2, 8192, 64};
    r.seg[3] = QnetGradSeg{out.b1, 1, net.h1, 9216, 0};
    r.seg[4] = QnetGradSeg{out.b2, 1, net.h2, 9280, 0};
    r.seg[5] = QnetGradSeg{out.b3, 1, QN_OUT, 9344, 0};
    r.nseg = 6;
    r.blocks = (int)blocks;
    r.stride = QG_P;
    r.clamp = clamp;
    r.partial = workspace;
    return launch_qnet_grad_reduce(r, s);
}

int launch_minimized_qnet_backward(const evg_mini_qnet& net, long long rows, const float* x, const float* gq, const evg_mini_qnet_grads& out,
                                   float* workspace, float clamp, int num_cu, void* stream) {
    MiniQnetGradArgs a;
    a.W = MiniQnetSet{net.w1[0], net.b1[0], net.w2[0], net.b2[0]};
    a.h1 = net.h1;
    a.final_relu = net.final_relu;
    a.rows = rows;
    a.x = x;
    a.gq = gq;
    a.partial = workspace;
    const long long blocks = qnet_grad_blocks(rows, num_cu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_mini_qnet_grad_kernel, dim3((unsigned)blocks), dim3(64 * QN_WAVES), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    QnetGradReduceArgs r;
    r.seg[0] = QnetGradSeg{out.w1, net.h1, QN_IN, 0, 64};
    r.seg[1] = QnetGradSeg{out.w2, MQ_OUT, net.h1, 4 * MG_CHUNK, MQ_H};
    r.seg[2] = QnetGradSeg{out.b1, 1, net.h1, 5 * MG_CHUNK, 0};
    r.seg[3] = QnetGradSeg{out.b2, 1, MQ_OUT, 5 * MG_CHUNK + 128, 0};
    for (int i = 4; i < 6; ++i) r.seg[i] = QnetGradSeg{nullptr, 0, 0, 0, 0};
    r.nseg = 4;
    r.blocks = (int)blocks;
    r.stride = MG_P;
    r.clamp = clamp;
    r.partial = workspace;
    return launch_qnet_grad_reduce(r, s);
}
