// qnet_body.inc -- the forward pass of one workgroup of the Smart_State Q network: the body that evg_qnet_kernel<EXPANDED> (qnet_kernels.inc; QN_GROUPED 0)
// and evg_qnet_pop_kernel<EXPANDED> (population_kernels.inc; QN_GROUPED 1) share.  It is program text included inside each kernel, not a function: as
// a __device__ __forceinline__ template the same statements leave the compiler with another schedule for the plain kernels (minimized_qnet_body.inc has
// the account), and those keep their instruction streams (profiles/r16_a_smart_population_isa.txt).  The including kernel defines, ahead of the include:
//   EXPANDED (its template parameter), a (QnetArgs), fixed / lds (its LDS), tid / lane / wave, seat (the seat slot of the compact layouts), W (the
//   weight set of this workgroup), and QN_GROUPED:
//     0  rows 0 .. a.rows - 1, groups of 16 dealt over the whole grid
//     1  the rows list[0 .. list_rows - 1] (const int*, long long) of one (seat, member), groups dealt over list_stride wavefronts (long long): a row's
//        inputs are read at, and its Q goes back to, the position in the caller's tensors that the list names (mq_list_row)
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
#if QN_GROUPED
    const long long R = list_rows;
#else
    const long long R = a.rows;
#endif
    const long long groups = (R + 15) >> 4;

#if QN_GROUPED
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += list_stride) {
        const long long r0 = g << 4;
        const bool va = r0 + col < R;
        const long long ra = va ? mq_list_row(list, r0 + col, a.rows) : 0;     // this lane's A row: the one its position in the list names
#else
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;                // this lane's A row
        const bool va = ra < R;
#endif
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
#if QN_GROUPED
            // the four rows of this lane's D fragment go back to the rows that positions r0 + row0 + r of the list name: lanes row0 + r hold them as
            // their A rows (one register kept across the layers; the plain kernel's 190 + 60 registers leave room for no more at 2 waves per SIMD)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ro = __shfl((int)ra, row0 + r, 64);
                if (col < QN_OUT && r0 + row0 + r < R) a.out[(long long)ro * QN_OUT + col] = q[r];
            }
#else
            if (col < QN_OUT)
#pragma unroll
                for (int r = 0; r < 4; ++r) qt[(row0 + r) * QN_OUT + col] = q[r];
            qn_wave_sync();
            const long long base = r0 * QN_OUT, end = R * QN_OUT;
            for (int i = lane; i < 16 * QN_OUT; i += 64)
                if (base + i < end) a.out[base + i] = qt[i];
#endif
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
#if QN_GROUPED
                if (r0 + row < R)                     // ... of the row that position r0 + row of the list names
                    reinterpret_cast<float4*>(a.out + ((long long)mq_list_row(list, r0 + row, a.rows) * S + seat) * 60)[c] =
                        reinterpret_cast<const float4*>(qt + row * 60)[c];
#else
                if (r0 + row < R)
                    reinterpret_cast<float4*>(a.out + ((r0 + row) * S + seat) * 60)[c] = reinterpret_cast<const float4*>(qt + row * 60)[c];
#endif
            }
        }
        qn_wave_sync();                               // the tiles are rewritten by the next group
    }
