// qnet_grad_body.inc -- the backward pass of one workgroup of the Smart_State Q network: the body that evg_qnet_grad_kernel (qnet_grad_kernels.inc;
// QG_GROUPED 0) and evg_poplearn_qnet_grad_kernel (pop_learn_kernels.inc; QG_GROUPED 1) share.  Program text included inside each kernel, not a function,
// for the reason qnet_body.inc gives: the plain kernel keeps its instruction stream.  The including kernel defines, ahead of the include:
//   a (QnetGradArgs), lds (its LDS, QG_LDS floats), W (the weight set of this workgroup), and QG_GROUPED:
//     0  rows 0 .. a.rows - 1, groups of 16 dealt over the whole grid; the partial goes to slot blockIdx.x
//     1  the rows list[0 .. list_rows - 1] (const int*, long long) of one member, groups dealt over list_stride wavefronts (long long); x and gq are
//        read at the rows the list names, the tail of the last group is masked against list_rows; the partial goes to slot part_slot (long long).
//        The four D-layout rows of a lane are taken by ds_bpermute from the lanes that hold them as A rows (lanes 0..15: kq 0, col = the position)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1, H2 = a.h2;
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
#if QG_GROUPED
    const long long R = list_rows, groups = (R + 15) >> 4;
#else
    const long long R = a.rows, groups = (R + 15) >> 4;
#endif
    const int arow = col * QN_HS + kq;
#if QG_GROUPED
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += list_stride) {
        const long long r0 = g << 4;
        const bool va = r0 + col < R;
        const long long ra = va ? mq_list_row(list, r0 + col, a.rows) : 0;     // this lane's A row: the one its position in the list names
#else
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;                // this lane's A row of the forward
        const bool va = ra < R;
#endif
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
#if QG_GROUPED
            const bool vr = r0 + row0 + st < R;       // the row that position r0 + row0 + st of the list names: lane row0 + st holds it as its A row
            const long long row = __shfl((int)ra, row0 + st, 64);
#pragma unroll
            for (int t = 0; t < 4; ++t) xb[st][t] = (vr && 16 * t + col < QN_IN) ? a.x[row * QN_IN + 16 * t + col] : 0.0f;
            gv[st] = (vr && col < QN_OUT) ? a.gq[row * QN_OUT + col] : 0.0f;
#else
            const long long row = r0 + row0 + st;
#pragma unroll
            for (int t = 0; t < 4; ++t) xb[st][t] = (row < R && 16 * t + col < QN_IN) ? a.x[row * QN_IN + 16 * t + col] : 0.0f;
            gv[st] = (row < R && col < QN_OUT) ? a.gq[row * QN_OUT + col] : 0.0f;
#endif
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
#if QG_GROUPED
    float* P = a.partial + part_slot * QG_P;
#else
    float* P = a.partial + (long long)blockIdx.x * QG_P;
#endif
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
