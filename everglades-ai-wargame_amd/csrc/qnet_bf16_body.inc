// qnet_bf16_body.inc -- the bf16 forward of one workgroup of the Smart_State Q network: the body that evg_qnet_bf16_kernel<EXPANDED>
// (qnet_bf16_kernels.inc; QB_GROUPED 0) and evg_qnet_pop_bf16_kernel<EXPANDED> (population_bf16_kernels.inc; QB_GROUPED 1) share.  It is program text
// included inside each kernel, not a function, for the reason qnet_body.inc gives: the plain kernels keep their instruction streams.  The including
// kernel defines, ahead of the include:
//   EXPANDED (its template parameter), a (QnetArgs), w1s / w2s / w3s (its LDS), tid / lane / wave, seat (the seat slot of the compact layouts), W (the
//   weight set of this workgroup), and QB_GROUPED:
//     0  rows 0 .. a.rows - 1, groups of 16 dealt over the whole grid
//     1  the rows list[0 .. list_rows - 1] (const int*, long long; list_rows >= 1) of one (seat, member), groups dealt over list_stride wavefronts
//        (long long).  A lane's row is column n of every tile and its results are that row's own, so ONE list entry per lane serves the loads and the
//        stores: a row's inputs are read at, and its Q goes back to, the position in the caller's tensors that the list names (mq_list_row).  A lane
//        past the end of the list takes the list's last entry and stores nothing -- the clamped address, then the select, of the plain form
    const int H1 = a.h1, H2 = a.h2, S = a.num_seats;
    qb_stage<QB_NATURAL>(w1s, W.w1, QN_IN, H1, EXPANDED ? QN_IN : 34, 4, 2, tid);
    if (!EXPANDED) qb_stage<QB_SWARM>(w1s + 8 * 64, W.w1, QN_IN, H1, QN_IN, 4, 1, tid);
    qb_stage<QB_CHAINED>(w2s, W.w2, H1, H2, H1, 4, 2, tid);
    qb_stage<QB_CHAINED>(w3s, W.w3, H2, QN_OUT, H2, 1, 2, tid);
    __syncthreads();

    const int n = lane & 15, q = lane >> 4;
    qb_bf8 w1f[4][EXPANDED ? 2 : 1], w2f[4][2], w3f[2];      // (the compact prefix's 8 fragments run once per 16 envs: read from LDS there)
    qn_f4 b1v[4], b2v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (EXPANDED) {
            w1f[t][0] = w1s[(2 * t) * 64 + lane];
            w1f[t][EXPANDED ? 1 : 0] = w1s[(2 * t + 1) * 64 + lane];
        } else {
            w1f[t][0] = w1s[(8 + t) * 64 + lane];
        }
        w2f[t][0] = w2s[(2 * t) * 64 + lane];
        w2f[t][1] = w2s[(2 * t + 1) * 64 + lane];
        b1v[t] = qb_bias(W.b1, H1, t, q);
        b2v[t] = qb_bias(W.b2, H2, t, q);
    }
    w3f[0] = w3s[lane];
    w3f[1] = w3s[64 + lane];
    const qn_f4 b3v = qb_bias(W.b3, QN_OUT, 0, q);

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
            qn_f4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = qb_mfma(w1f[t][EXPANDED ? 1 : 0], x1, qb_mfma(w1f[t][0], x0, b1v[t]));
            const qn_f4 out = qb_smart_tail(acc, w2f, w3f, b2v, b3v, H1, H2, a.final_relu, QB_Q);
            qb_store_q<QN_OUT>(a.out + rc * QN_OUT + 4 * QB_Q, out, QB_Q, va);
        } else {
            const long long vr = rc * S + seat;          // the row of (env, seat) in [R][S][...]
            const float* sh = a.in0 + vr * 34;
            const float* sw = a.in1 + vr * (12 * 13);
            qb_bf4 xs[12];                                // every swarm's features, in flight from here on
#pragma unroll
            for (int s = 0; s < 12; ++s) xs[s] = qb_load_swarm(sw + 13 * s, QB_Q, va);
            const qb_bf8 p0 = qb_load8(sh, 8 * QB_Q, 34, va), p1 = qb_load8(sh, 32 + 8 * QB_Q, 34, va);
            qn_f4 pre[4];                                 // b1 + the 34 shared terms, once per env
#pragma unroll
            for (int t = 0; t < 4; ++t) pre[t] = qb_mfma(w1s[(2 * t + 1) * 64 + lane], p1, qb_mfma(w1s[(2 * t) * 64 + lane], p0, b1v[t]));
            float* o = a.out + vr * (12 * QN_OUT) + 4 * QB_Q;
#pragma unroll
            for (int s = 0; s < 12; ++s) {
#if QB_GROUPED
                asm volatile("" : "+v"(qv));      // (... and once per swarm)
#endif
                const qb_bf8 xb = qb_swarm_frag(xs[s], s, QB_Q);
                qn_f4 acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = qb_mfma(w1f[t][0], xb, pre[t]);
                const qn_f4 out = qb_smart_tail(acc, w2f, w3f, b2v, b3v, H1, H2, a.final_relu, QB_Q);
                qb_store_q<QN_OUT>(o + s * QN_OUT, out, QB_Q, va);
            }
        }
    }
#undef QB_Q
