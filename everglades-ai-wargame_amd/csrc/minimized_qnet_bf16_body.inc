// minimized_qnet_bf16_body.inc -- the bf16 forward of one workgroup of the Minimized Q network: the body that evg_mini_qnet_bf16_kernel<EXPANDED>
// (qnet_bf16_kernels.inc; QB_GROUPED 0) and evg_mini_qnet_pop_bf16_kernel<EXPANDED> (population_bf16_kernels.inc; QB_GROUPED 1) share.  It is program text
// included inside each kernel, not a function, for the reason minimized_qnet_body.inc gives: the plain kernels keep their instruction streams.  The including
// kernel defines, ahead of the include:
//   EXPANDED (its template parameter), a (MiniQnetArgs), w1s / w2s / b1s (its LDS), tid / lane / wave, seat (the seat slot of the compact layouts), W (the
//   weight set of this workgroup), and QB_GROUPED:
//     0  rows 0 .. a.rows - 1, groups of 16 dealt over the whole grid
//     1  the rows list[0 .. list_rows - 1] (const int*, long long; list_rows >= 1) of one (seat, member), groups dealt over list_stride wavefronts
//        (long long).  A lane's row is column n of every tile and its results are that row's own, so ONE list entry per lane serves the loads and the
//        stores: a row's inputs are read at, and its Q goes back to, the position in the caller's tensors that the list names (mq_list_row).  A lane
//        past the end of the list takes the list's last entry and stores nothing -- the clamped address, then the select, of the plain form
    const int H1 = a.h1, S = a.num_seats;
    const int nt = (H1 + 15) >> 4;                        // column tiles of the hidden layer
    qb_stage<QB_NATURAL>(w1s, W.w1, QN_IN, H1, EXPANDED ? QN_IN : 34, nt, 2, tid);
    if (!EXPANDED) qb_stage<QB_SWARM>(w1s + 2 * MQ_TILES * 64, W.w1, QN_IN, H1, QN_IN, nt, 1, tid);
    qb_stage<QB_CHAINED>(w2s, W.w2, H1, MQ_OUT, H1, 1, MQ_TILES / 2, tid);
    for (int i = tid; i < MQ_H; i += 64 * QN_WAVES) b1s[i] = i < H1 ? W.b1[i] : 0.0f;
    __syncthreads();

    const int n = lane & 15, q = lane >> 4;
    qb_bf8 swf[EXPANDED ? 1 : MQ_TILES], w2f[MQ_TILES / 2];   // (the other layer-1 fragments are read from LDS at every use)
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t)
        if (!EXPANDED && t < nt) swf[t] = w1s[(2 * MQ_TILES + t) * 64 + lane];
#pragma unroll
    for (int u = 0; u < MQ_TILES / 2; ++u) w2f[u] = w2s[u * 64 + lane];
    const qn_f4 b2v = qb_bias(W.b2, MQ_OUT, 0, q);
    const qn_f4 zero = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};

#if QB_GROUPED
    const long long R = list_rows, groups = (R + 15) >> 4;
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += list_stride) {
        const long long pa = (g << 4) + n;                // this lane's position in the list: column n of every tile
        const bool va = pa < R;
        // the row this lane reads and writes: the one its position names, or (past the end) the one the list's last entry names, whose values it drops
        const long long rc = mq_list_row(list, va ? pa : R - 1, a.rows);
        // (the lane's quarter, opaque once per group: the masks that depend on it are recomputed inside the group instead of being kept across the loop as
        // SGPR pairs, which spilled; the plain form keeps its statements, token for token)
        int qv = q;
        asm volatile("" : "+v"(qv));
#define QB_Q qv
#else
    const long long R = a.rows, groups = (R + 15) >> 4;
    for (long long g = (long long)blockIdx.x * QN_WAVES + wave; g < groups; g += (long long)gridDim.x * QN_WAVES) {
        const long long ra = (g << 4) + n;                // this lane's row: column n of every tile
        const bool va = ra < R;
        const long long rc = va ? ra : R - 1;             // the row this lane reads: its own, or (past the end) the last one, whose values it drops
#define QB_Q q
#endif
        if (EXPANDED) {
            const float* x = a.in0 + rc * QN_IN;
            const qb_bf8 x0 = qb_load8(x, 8 * QB_Q, QN_IN, va), x1 = qb_load8(x, 32 + 8 * QB_Q, QN_IN, va);
            qn_f4 acc[MQ_TILES];
#pragma unroll
            for (int t = 0; t < MQ_TILES; ++t) {
                acc[t] = zero;
                if (t < nt)
                    acc[t] = qb_mfma(w1s[(2 * t + 1) * 64 + lane], x1,
                                     qb_mfma(w1s[(2 * t) * 64 + lane], x0, *reinterpret_cast<const qn_f4*>(b1s + 16 * t + 4 * QB_Q)));
            }
            const qn_f4 out = qb_mini_tail(acc, w2f, b2v, H1, nt, a.final_relu, QB_Q);
            qb_store_q<MQ_OUT>(a.out + rc * MQ_OUT + 4 * QB_Q, out, QB_Q, va);
        } else {
            const long long vr = rc * S + seat;          // the row of (env, seat) in [R][S][...]
            const float* sh = a.in0 + vr * 34;
            const float* sw = a.in1 + vr * (12 * 13);
            qb_bf4 xs[12];                                // every swarm's features, in flight from here on
#pragma unroll
            for (int s = 0; s < 12; ++s) xs[s] = qb_load_swarm(sw + 13 * s, QB_Q, va);
            const qb_bf8 p0 = qb_load8(sh, 8 * QB_Q, 34, va), p1 = qb_load8(sh, 32 + 8 * QB_Q, 34, va);
            qn_f4 pre[MQ_TILES];                          // b1 + the 34 shared terms, once per env
#pragma unroll
            for (int t = 0; t < MQ_TILES; ++t) {
                pre[t] = zero;
                if (t < nt)
                    pre[t] = qb_mfma(w1s[(2 * t + 1) * 64 + lane], p1,
                                     qb_mfma(w1s[(2 * t) * 64 + lane], p0, *reinterpret_cast<const qn_f4*>(b1s + 16 * t + 4 * QB_Q)));
            }
            float* o = a.out + vr * (12 * MQ_OUT) + 4 * QB_Q;
#pragma unroll
            for (int s = 0; s < 12; ++s) {
#if QB_GROUPED
                asm volatile("" : "+v"(qv));      // (... and once per swarm)
#endif
                const qb_bf8 xb = qb_swarm_frag(xs[s], s, QB_Q);
                qn_f4 acc[MQ_TILES];
#pragma unroll
                for (int t = 0; t < MQ_TILES; ++t) {
                    acc[t] = zero;
                    if (t < nt) acc[t] = qb_mfma(swf[t], xb, pre[t]);
                }
                const qn_f4 out = qb_mini_tail(acc, w2f, b2v, H1, nt, a.final_relu, QB_Q);
                qb_store_q<MQ_OUT>(o + s * MQ_OUT, out, QB_Q, va);
            }
        }
    }
#undef QB_Q
