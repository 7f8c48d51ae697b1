// minimized_qnet_body.inc -- the forward pass of one workgroup of the Minimized Q network: the body that evg_mini_qnet_kernel<EXPANDED>
// (minimized_qnet.inc; MQ_GROUPED 0) and evg_mini_qnet_pop_kernel<EXPANDED> (population_kernels.inc; MQ_GROUPED 1) share.  It is program text included
// inside each kernel, not a function: wrapped in a __device__ __forceinline__ template, the same statements leave the compiler with another schedule for
// the two plain kernels (profiles/r15_a_population_isa.txt), and those keep their instruction streams.  The including kernel defines, ahead of the include:
//   EXPANDED (its template parameter), a (MiniQnetArgs), wl / tiles (its LDS), tid / lane / wave, seat (the seat slot of the compact layouts), W (the
//   weight set of this workgroup), and MQ_GROUPED:
//     0  rows 0 .. a.rows - 1, groups of 16 dealt over the whole grid
//     1  the rows list[0 .. list_rows - 1] (const int*, long long) of one (seat, member), groups dealt over list_stride wavefronts (long long): a row's
//        inputs are read at, and its Q goes back to, the position in the caller's tensors that the list names (mq_list_row)
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
#if MQ_GROUPED
    const long long R = list_rows;
#else
    const long long R = a.rows;
#endif
    const long long groups = (R + 15) >> 4;

#if MQ_GROUPED
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += list_stride) {
        const long long r0 = g << 4;
        const bool va = r0 + col < R;
        const long long ra = va ? mq_list_row(list, r0 + col, a.rows) : 0;     // this lane's A row: the one its position in the list names
        int ro[4];                                    // ... and where the four rows of this lane's D fragment go back to
#pragma unroll
        for (int r = 0; r < 4; ++r) ro[r] = r0 + row0 + r < R ? mq_list_row(list, r0 + row0 + r, a.rows) : 0;
#define MQ_OUT_ROW(r) ((long long)ro[r])
#else
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long r0 = g << 4;
        const long long ra = r0 + col;                // this lane's A row
        const bool va = ra < R;
#define MQ_OUT_ROW(r) (r0 + row0 + r)
#endif
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
                    if (r0 + row0 + r < R) a.out[MQ_OUT_ROW(r) * MQ_OUT + col] = q[r];
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
                        if (r0 + row0 + r < R) a.out[(MQ_OUT_ROW(r) * S + seat) * (12 * MQ_OUT) + s * MQ_OUT + col] = q[r];
                qn_wave_sync();                       // the tile is rewritten by the next swarm
            }
        }
        qn_wave_sync();                               // the tile is rewritten by the next group
    }
#undef MQ_OUT_ROW
