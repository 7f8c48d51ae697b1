// minimized_qnet_grad_body.inc -- the backward pass of one workgroup of the Minimized Q network: the body that evg_mini_qnet_grad_kernel
// (qnet_grad_kernels.inc; QG_GROUPED 0) and evg_poplearn_mini_qnet_grad_kernel (pop_learn_kernels.inc; QG_GROUPED 1) share, as qnet_grad_body.inc is for
// the Smart_State network.  The including kernel defines a (MiniQnetGradArgs), lds, W and QG_GROUPED (0: the plain rows; 1: list, list_rows,
// list_stride, part_slot -- qnet_grad_body.inc has the account).
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1;
    const int nt = (H1 + 15) >> 4;                     // column tiles of the hidden layer
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

#if QG_GROUPED
    const long long R = list_rows, groups = (R + 15) >> 4;
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += list_stride) {
        const long long r0 = g << 4;
        const bool va = r0 + col < R;
        const long long ra = va ? mq_list_row(list, r0 + col, a.rows) : 0;     // this lane's A row: the one its position in the list names
#else
    const long long R = a.rows, groups = (R + 15) >> 4;
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;
        const bool va = ra < R;
#endif
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
#if QG_GROUPED
            const bool vr = r0 + row0 + st < R;       // the row that position r0 + row0 + st of the list names: lane row0 + st holds it as its A row
            const long long row = __shfl((int)ra, row0 + st, 64);
#pragma unroll
            for (int t = 0; t < 4; ++t) xb[st][t] = (vr && 16 * t + col < QN_IN) ? a.x[row * QN_IN + 16 * t + col] : 0.0f;
            gv[st] = (vr && col < MQ_OUT) ? a.gq[row * MQ_OUT + col] : 0.0f;
#else
            const long long row = r0 + row0 + st;
#pragma unroll
            for (int t = 0; t < 4; ++t) xb[st][t] = (row < R && 16 * t + col < QN_IN) ? a.x[row * QN_IN + 16 * t + col] : 0.0f;
            gv[st] = (row < R && col < MQ_OUT) ? a.gq[row * MQ_OUT + col] : 0.0f;
#endif
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
#if QG_GROUPED
    float* P = a.partial + part_slot * MG_P;
#else
    float* P = a.partial + (long long)blockIdx.x * MG_P;
#endif
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
