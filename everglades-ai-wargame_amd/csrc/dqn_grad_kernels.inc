// dqn_grad_kernels.inc -- the backward pass of the agents/DQN family's Q network (include/evg_dqn_grad.h, evg_dqn_qnet_backward): the parameter
// gradients of optimize_model's policy forward for QNetwork(105 -> h1 <= 528 -> 132).  Included by evg_kernels.hip (namespace evg) under EVG_DQN_GRAD
// (with EVG_DQN), after dqn_kernels.inc, whose constants, staging (DqnArgs, dqn_fetch / dqn_commit) and numeric contract it shares; libevg_dqngrad.so
// only.
//
//   evg_dqn_delta_kernel<SPLIT>   row-parallel, the forward's structure: a1 (the exact chain) and d1 = (W2^T d2) * (a1 > 0) -> workspace [rows][HP]
//   evg_dqn_wgrad_kernel          tile-parallel: a wavefront owns one hidden tile's 9 tiles of gW2 and 7 of gW1 and runs down the rows (the K of an
//                                 fp32-MFMA GEMM); the rows are cut into slices, one workgroup column per slice
//   evg_dqn_grad_reduce_kernel    more than one slice: the slices' partial sums added in ascending slice order, the clamp
//
// A parameter set is 503 KB: no workgroup can keep one (minimized_qnet_grad_body.inc's way), so the weight gradients are computed the other way
// round.  Both GEMMs have the rows as K, and every operand of a k-step is a fragment V[r0 + (lane >> 4)][c0 + (lane & 15)] of a row-major matrix:
//
//   gW2[o][j] = sum_r d2[r][o] a1[r][j]     A = d2 (M = o), B = a1 (N = j)        D register i = gW2[16 ot + 4 (lane >> 4) + i][16 jt + (lane & 15)]
//   gW1[j][k] = sum_r d1[r][j] x[r][k]      A = d1 (M = j), B = x  (N = k)        D register i = gW1[16 jt + 4 (lane >> 4) + i][16 kt + (lane & 15)]
//
// so a wavefront with hidden tile jt needs, per k-step, ONE a1 fragment and ONE d1 fragment of its own (shared by its 9 and 7 tiles) and the 9 d2
// and 7 x fragments every wavefront of the workgroup reads from the same staged block.  The bias gradients are per-lane sums of the A fragments
// (gb1: d1; gb2: d2, hidden tile 0's wavefront only), combined over the four k lanes in ascending order at the end.
//
// Padding is by selection, as in the forward: d2's columns 132..143 and x's 105..111 are zeros in LDS written once, rows past a slice's end are
// stored as zeros, the delta kernel stores a1 = d1 = 0 for units h1..HP-1, and nothing outside the nn.Linear shapes is written.

constexpr int DG_KB = 32;                                // rows per staged block of the weight-gradient kernel (8 k-steps)
constexpr int DG_D2S = 144, DG_XS = 112, DG_HS = 80;     // LDS row strides: all = 16 mod 32, so a k-step's 2 x 16 lanes of a ds_read_b32 group fall
                                                         // into 32 banks
constexpr int DG_KO = DQ_OUT / 4;                        // d1's k-steps: 132 = 4 x 33 outputs, no padded k
constexpr int DG_XT = 7;                                 // gW1's column tiles (112 columns)
constexpr int DG_NQ = (DG_KB * (DQ_OUT / 4) + 255) / 256;    // staged float4 per lane: gq / q block (32 x 33 = 1 056 -> 5)
constexpr int DG_NX = (DG_KB * DQ_IN + 255) / 256;           // staged floats per lane: x block (32 x 105 = 3 360 -> 14)
constexpr int DG_NH = (DG_KB * 16) / 256;                    // staged float4 per lane: a1 / d1 block (32 rows x 64 columns -> 2)
static_assert(DQ_OUT % 4 == 0 && DG_KB % 4 == 0 && DG_KB * 16 == 256 * DG_NH, "the staging loops");

struct DqnGradArgs {
    DqnArgs net;                // the forward's argument set: parameters, h1, final_relu, rows, x (float32 rows, stride 105)
    const float* q;             // [rows][132] or NULL (final_relu == 0)
    const float* gq;            // [rows][132]
    float* a1;                  // workspace: [rows][HP]
    float* d1;                  // workspace: [rows][HP]
    float* part;                // workspace: [S][257 HP + 144], S > 1 only
    float* gw1;
    float* gb1;
    float* gw2;
    float* gb2;
    int HP, NT, CG, S;          // h1 rounded up to 16, hidden tiles, workgroups per slice (4 hidden tiles each), slices
    long long RS;               // rows per slice (a multiple of DG_KB)
    float clamp;
};

__device__ __forceinline__ float dg_clamp(float v, float c) { return c > 0.0f ? fminf(fmaxf(v, -c), c) : v; }

// ---------------------------------------------------------------------------------------------
// delta kernel.  SPLIT: a workgroup pass is ONE group of 16 rows and wavefronts 0..2 take one column tile of the chunk each (wavefront 3 only stages);
// otherwise a pass is 64 rows, a wavefront owns 16 of them and runs the chunk's three column tiles side by side (three independent accumulator
// chains).  Per chunk and tile: layer 1's chain exactly as evg_dqn_qnet_kernel runs it (acc = b1, 27 k-steps over the staged W1 rows), then d1's tile
// = d2 [16 x 132] . W2[:, tile] over 33 k-steps of the staged W2 columns, read as B fragments w2s[o][unit]; both tiles leave in the D layout, so the
// mask a1 > 0 is elementwise in registers.
// ---------------------------------------------------------------------------------------------
template <bool SPLIT>
__global__ void __launch_bounds__(256) evg_dqn_delta_kernel(DqnGradArgs g) {
    __shared__ float w1s[DQ_C * DQ_W1S];
    __shared__ float w2s[16 * DQ_OT * DQ_W2S];
    __shared__ float b1s[DQ_C];
    const DqnArgs& a = g.net;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4, row0 = 4 * kq;
    const int H1 = a.h1, HP = g.HP;
    const int chunks = (H1 + DQ_C - 1) / DQ_C;
    const long long R = a.rows;
    constexpr int RB = SPLIT ? 16 : 64, TI = SPLIT ? 1 : DQ_CT;
    const long long passes = (R + RB - 1) / RB;
    const bool work = !SPLIT || wave < DQ_CT;          // (wave-uniform)
    const float* __restrict__ xin = static_cast<const float*>(a.x);

    for (long long pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const long long rbase = pass * RB + (SPLIT ? 0 : 16 * wave);
        const long long ra = rbase + col;
        const bool va = ra < R;
        const long long rl = va ? ra : R - 1;          // (a clamped row and column: every load is inside the buffers)
        // ---- this lane's A fragments: x[row l & 15][4 s + (l >> 4)] as the forward reads them, and d2[row l & 15][4 s + (l >> 4)], formed on load
        float xa[DQ_KX], d2a[DG_KO];
        {
            const float* x = xin + rl * DQ_IN;
#pragma unroll
            for (int s = 0; s < DQ_KX; ++s) {
                const int k = 4 * s + kq;
                const float v = x[4 * s + 3 < DQ_IN ? k : min(k, DQ_IN - 1)];
                xa[s] = (va && (4 * s + 3 < DQ_IN || k < DQ_IN)) ? v : 0.0f;
            }
            const float* gq = g.gq + rl * DQ_OUT;
            const float* q = (a.final_relu ? g.q : g.gq) + rl * DQ_OUT;
#pragma unroll
            for (int s = 0; s < DG_KO; ++s) {
                const float v = gq[4 * s + kq], m = q[4 * s + kq];
                d2a[s] = (va && (!a.final_relu || m > 0.0f)) ? v : 0.0f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        DqnStage st;
        dqn_fetch(st, a, 0, tid);

        int c = 0;                                     // (h1 >= 1: at least one chunk)
#pragma unroll 1
        do {
            const int c0 = c * DQ_C;
            __syncthreads();                           // every wavefront is done with the chunk that LDS holds
            dqn_commit(st, c0, H1, w1s, w2s, b1s, tid);
            __syncthreads();
            if (c + 1 < chunks) dqn_fetch(st, a, c0 + DQ_C, tid);      // in flight during this chunk's MFMAs
            __builtin_amdgcn_sched_barrier(0);
            if (work) {
                qn_f4 acc1[TI], accd[TI];
                int t[TI];
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    t[i] = SPLIT ? wave : i;
                    const float b = b1s[16 * t[i] + col];
                    acc1[i] = qn_f4{b, b, b, b};
                    accd[i] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};
                }
#pragma unroll
                for (int s = 0; s < DQ_KX; ++s)
#pragma unroll
                    for (int i = 0; i < TI; ++i) acc1[i] = qn_mfma(xa[s], w1s[(16 * t[i] + col) * DQ_W1S + 4 * s + kq], acc1[i]);
#pragma unroll
                for (int s = 0; s < DG_KO; ++s)
#pragma unroll
                    for (int i = 0; i < TI; ++i) accd[i] = qn_mfma(d2a[s], w2s[(4 * s + kq) * DQ_W2S + 16 * t[i] + col], accd[i]);
                // ---- a1 = ReLU of the chain, d1 masked by it; a unit >= h1 is an exact zero in both whatever its accumulators hold
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int unit = c0 + 16 * t[i] + col;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const long long row = rbase + row0 + r;
                        const float h = unit < H1 ? qn_relu(acc1[i][r]) : 0.0f;
                        const float d = h > 0.0f ? accd[i][r] : 0.0f;
                        if (row < R && unit < HP) {
                            g.a1[row * HP + unit] = h;
                            g.d1[row * HP + unit] = d;
                        }
                    }
                }
            }
        } while (++c < chunks);
    }
}

// ---------------------------------------------------------------------------------------------
// weight-gradient kernel.  Workgroup (cg, s): hidden tiles 4 cg .. 4 cg + 3 (one per wavefront), rows [s RS, min(rows, (s + 1) RS)).  Per block of
// DG_KB rows the workgroup stages d2 (formed from gq and q, float4 loads), x (dword loads: a row is 420 bytes), and its 64 columns of a1 and d1
// (float4 loads) -- the next block is fetched into registers while this one is computed.
// ---------------------------------------------------------------------------------------------
struct DqnGradStage {
    float gq[DG_NQ][4], q[DG_NQ][4], a1[DG_NH][4], d1[DG_NH][4], x[DG_NX];
};

__device__ __forceinline__ void dg_fetch(DqnGradStage& s, const DqnGradArgs& g, long long rb, long long rend, int j0, int tid) {
    asm volatile("" : "+v"(tid));                      // (as in dqn_fetch: the indices are recomputed, not kept in registers across the kernel)
    const long long last = rend - 1;
    const float4* gq4 = reinterpret_cast<const float4*>(g.gq);
    const float4* q4 = reinterpret_cast<const float4*>(g.net.final_relu ? g.q : g.gq);
#pragma unroll
    for (int it = 0; it < DG_NQ; ++it) {
        const int f = min(tid + 256 * it, DG_KB * (DQ_OUT / 4) - 1), r = f / (DQ_OUT / 4), c4 = f - (DQ_OUT / 4) * r;
        const long long at = min(rb + r, last) * (DQ_OUT / 4) + c4;
        const float4 v = gq4[at], m = q4[at];
        s.gq[it][0] = v.x; s.gq[it][1] = v.y; s.gq[it][2] = v.z; s.gq[it][3] = v.w;
        s.q[it][0] = m.x; s.q[it][1] = m.y; s.q[it][2] = m.z; s.q[it][3] = m.w;
    }
#pragma unroll
    for (int it = 0; it < DG_NX; ++it) {
        const int e = min(tid + 256 * it, DG_KB * DQ_IN - 1), r = e / DQ_IN, k = e - DQ_IN * r;
        s.x[it] = static_cast<const float*>(g.net.x)[min(rb + r, last) * DQ_IN + k];
    }
#pragma unroll
    for (int it = 0; it < DG_NH; ++it) {
        const int f = tid + 256 * it, r = f >> 4, c4 = f & 15;
        const int colu = min(j0 + 4 * c4, g.HP - 4);
        const long long at = (min(rb + r, last) * g.HP + colu) >> 2;
        const float4 v = reinterpret_cast<const float4*>(g.a1)[at], d = reinterpret_cast<const float4*>(g.d1)[at];
        s.a1[it][0] = v.x; s.a1[it][1] = v.y; s.a1[it][2] = v.z; s.a1[it][3] = v.w;
        s.d1[it][0] = d.x; s.d1[it][1] = d.y; s.d1[it][2] = d.z; s.d1[it][3] = d.w;
    }
}

__device__ __forceinline__ void dg_commit(const DqnGradStage& s, const DqnGradArgs& g, long long rb, long long rend, int j0, float* __restrict__ d2s,
                                          float* __restrict__ xs, float* __restrict__ a1s, float* __restrict__ d1s, int tid) {
    asm volatile("" : "+v"(tid));
    const bool fr = g.net.final_relu != 0;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int it = 0; it < DG_NQ; ++it) {
        const int f = tid + 256 * it, r = f / (DQ_OUT / 4), c4 = f - (DQ_OUT / 4) * r;
        if (f < DG_KB * (DQ_OUT / 4)) {
            const bool live = rb + r < rend;
            float4 v;
            v.x = (live && (!fr || s.q[it][0] > 0.0f)) ? s.gq[it][0] : 0.0f;
            v.y = (live && (!fr || s.q[it][1] > 0.0f)) ? s.gq[it][1] : 0.0f;
            v.z = (live && (!fr || s.q[it][2] > 0.0f)) ? s.gq[it][2] : 0.0f;
            v.w = (live && (!fr || s.q[it][3] > 0.0f)) ? s.gq[it][3] : 0.0f;
            *reinterpret_cast<float4*>(&d2s[r * DG_D2S + 4 * c4]) = v;
        }
    }
#pragma unroll
    for (int it = 0; it < DG_NX; ++it) {
        const int e = tid + 256 * it, r = e / DQ_IN, k = e - DQ_IN * r;
        if (e < DG_KB * DQ_IN) xs[r * DG_XS + k] = rb + r < rend ? s.x[it] : 0.0f;
    }
#pragma unroll
    for (int it = 0; it < DG_NH; ++it) {
        const int f = tid + 256 * it, r = f >> 4, c4 = f & 15;
        const bool live = rb + r < rend && j0 + 4 * c4 < g.HP;
        *reinterpret_cast<float4*>(&a1s[r * DG_HS + 4 * c4]) = live ? make_float4(s.a1[it][0], s.a1[it][1], s.a1[it][2], s.a1[it][3]) : zero;
        *reinterpret_cast<float4*>(&d1s[r * DG_HS + 4 * c4]) = live ? make_float4(s.d1[it][0], s.d1[it][1], s.d1[it][2], s.d1[it][3]) : zero;
    }
}

// the four k lanes' sums of column `col`, added in ascending k-lane order, in every lane
__device__ __forceinline__ float dg_sum_k(float v, int col) {
    const float s0 = __shfl(v, col), s1 = __shfl(v, col + 16), s2 = __shfl(v, col + 32), s3 = __shfl(v, col + 48);
    return ((s0 + s1) + s2) + s3;
}

__global__ void __launch_bounds__(256) evg_dqn_wgrad_kernel(DqnGradArgs g) {
    __shared__ __attribute__((aligned(16))) float d2s[DG_KB * DG_D2S];
    __shared__ __attribute__((aligned(16))) float xs[DG_KB * DG_XS];
    __shared__ __attribute__((aligned(16))) float a1s[DG_KB * DG_HS];
    __shared__ __attribute__((aligned(16))) float d1s[DG_KB * DG_HS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int cg = (int)(blockIdx.x % (unsigned)g.CG), sl = (int)(blockIdx.x / (unsigned)g.CG);
    const int j0 = 64 * cg, jt = 4 * cg + wave;
    const bool work = jt < g.NT, bias2 = jt == 0;      // (wave-uniform)
    const int H1 = g.net.h1, HP = g.HP;
    const long long rbeg = sl * g.RS, rend = min(g.net.rows, rbeg + g.RS);

    // the padded columns of d2 and x: zeros written once, never rewritten by dg_commit
    for (int i = tid; i < DG_KB * (DG_D2S - DQ_OUT); i += 256) d2s[(i / (DG_D2S - DQ_OUT)) * DG_D2S + DQ_OUT + i % (DG_D2S - DQ_OUT)] = 0.0f;
    for (int i = tid; i < DG_KB * (DG_XS - DQ_IN); i += 256) xs[(i / (DG_XS - DQ_IN)) * DG_XS + DQ_IN + i % (DG_XS - DQ_IN)] = 0.0f;

    qn_f4 acc2[DQ_OT], acc1[DG_XT];
    float sb2[DQ_OT], sb1 = 0.0f;
#pragma unroll
    for (int o = 0; o < DQ_OT; ++o) { acc2[o] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f}; sb2[o] = 0.0f; }
#pragma unroll
    for (int i = 0; i < DG_XT; ++i) acc1[i] = qn_f4{0.0f, 0.0f, 0.0f, 0.0f};

    DqnGradStage st;
    dg_fetch(st, g, rbeg, rend, j0, tid);
#pragma unroll 1
    for (long long rb = rbeg; rb < rend; rb += DG_KB) {
        __syncthreads();                               // every wavefront is done with the block that LDS holds
        dg_commit(st, g, rb, rend, j0, d2s, xs, a1s, d1s, tid);
        __syncthreads();
        if (rb + DG_KB < rend) dg_fetch(st, g, rb + DG_KB, rend, j0, tid);     // in flight during this block's MFMAs
        __builtin_amdgcn_sched_barrier(0);
        if (work) {
#pragma unroll 2
            for (int ks = 0; ks < DG_KB / 4; ++ks) {
                const int row = 4 * ks + kq;
                const float af = a1s[row * DG_HS + 16 * wave + col], df = d1s[row * DG_HS + 16 * wave + col];
                sb1 += df;
#pragma unroll
                for (int o = 0; o < DQ_OT; ++o) {
                    const float d2f = d2s[row * DG_D2S + 16 * o + col];
                    acc2[o] = qn_mfma(d2f, af, acc2[o]);
                    if (bias2) sb2[o] += d2f;
                }
#pragma unroll
                for (int i = 0; i < DG_XT; ++i) acc1[i] = qn_mfma(df, xs[row * DG_XS + 16 * i + col], acc1[i]);
            }
        }
    }
    if (!work) return;

    // ---- the accumulators leave: one slice -> the gradients themselves (clamped, the nn.Linear shapes only); more -> this slice's partial
    const bool final = g.S == 1;
    float* part = g.part + (final ? 0 : (long long)sl * (257LL * HP + 144));
    float* pw2 = part;                                 // [144][HP]
    float* pw1 = part + 144LL * HP;                    // [HP][112]
    float* pb2 = pw1 + 112LL * HP;                     // [144]
    float* pb1 = pb2 + 144;                            // [HP]
    const int unit = 16 * jt + col;
#pragma unroll
    for (int o = 0; o < DQ_OT; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int out = 16 * o + 4 * kq + r;
            if (final) {
                if (out < DQ_OUT && unit < H1) g.gw2[out * H1 + unit] = dg_clamp(acc2[o][r], g.clamp);
            } else {
                pw2[out * HP + unit] = acc2[o][r];
            }
        }
#pragma unroll
    for (int i = 0; i < DG_XT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * jt + 4 * kq + r, k = 16 * i + col;
            if (final) {
                if (u < H1 && k < DQ_IN) g.gw1[u * DQ_IN + k] = dg_clamp(acc1[i][r], g.clamp);
            } else {
                pw1[u * DG_XS + k] = acc1[i][r];
            }
        }
    const float b1sum = dg_sum_k(sb1, col);
    if (kq == 0) {
        if (final) {
            if (unit < H1) g.gb1[unit] = dg_clamp(b1sum, g.clamp);
        } else {
            pb1[unit] = b1sum;
        }
    }
    if (bias2) {
#pragma unroll
        for (int o = 0; o < DQ_OT; ++o) {
            const float b2sum = dg_sum_k(sb2[o], col);
            if (kq == 0) {
                if (final) {
                    if (16 * o + col < DQ_OUT) g.gb2[16 * o + col] = dg_clamp(b2sum, g.clamp);
                } else {
                    pb2[16 * o + col] = b2sum;
                }
            }
        }
    }
}

// the slices' partial sums, added in ascending slice order; one thread per gradient element (gW2, gW1, gb2, gb1 in this order)
__global__ void __launch_bounds__(256) evg_dqn_grad_reduce_kernel(DqnGradArgs g) {
    const int H1 = g.net.h1, HP = g.HP;
    const int n2 = DQ_OUT * H1, n1 = H1 * DQ_IN, total = n2 + n1 + DQ_OUT + H1;
    const long long pstride = 257LL * HP + 144;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        long long src;
        float* dst;
        if (e < n2) {
            const int o = e / H1, j = e - H1 * o;
            src = (long long)o * HP + j; dst = g.gw2 + e;
        } else if (e < n2 + n1) {
            const int i = e - n2, j = i / DQ_IN, k = i - DQ_IN * j;
            src = 144LL * HP + (long long)j * DG_XS + k; dst = g.gw1 + i;
        } else if (e < n2 + n1 + DQ_OUT) {
            const int o = e - n2 - n1;
            src = 256LL * HP + o; dst = g.gb2 + o;
        } else {
            const int j = e - n2 - n1 - DQ_OUT;
            src = 256LL * HP + 144 + j; dst = g.gb1 + j;
        }
        float sum = g.part[src];
        for (int s = 1; s < g.S; ++s) sum += g.part[s * pstride + src];
        *dst = dg_clamp(sum, g.clamp);
    }
}

// the slices of a call: S0 = EVG_DQN_GRAD_SLICES(rows) equal slices of RS rows, RS rounded up to the staged block; S = the slices that are not empty
static void dqn_grad_slices(long long rows, int& S, long long& RS) {
    const long long S0 = EVG_DQN_GRAD_SLICES(rows);
    RS = ((rows + S0 - 1) / S0 + DG_KB - 1) / DG_KB * DG_KB;
    S = (int)((rows + RS - 1) / RS);
}

int launch_dqn_qnet_backward(const evg_dqn_net& net, long long rows, const float* x, const float* q, const float* gq, const evg_dqn_grads& out,
                             float* workspace, float clamp, void* stream) {
    static_assert(EVG_DQN_GRAD_TINY_ROWS / 16 <= EVG_DQN_GRAD_MAX_BLOCKS && EVG_DQN_GRAD_SLICE_ROWS % DG_KB == 0, "the split form's grid is under the cap");
    DqnGradArgs g;
    g.net = DqnArgs{net.w1, net.b1, net.w2, net.b2, net.h1, net.final_relu, rows, x, DQ_IN, 0, nullptr};
    g.q = q; g.gq = gq;
    g.HP = (int)EVG_DQN_GRAD_HP(net.h1); g.NT = g.HP / 16; g.CG = (g.NT + 3) / 4;
    dqn_grad_slices(rows, g.S, g.RS);
    g.a1 = workspace; g.d1 = workspace + rows * g.HP; g.part = workspace + 2 * rows * g.HP;
    g.gw1 = out.w1; g.gb1 = out.b1; g.gw2 = out.w2; g.gb2 = out.b2;
    g.clamp = clamp;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (rows <= EVG_DQN_GRAD_TINY_ROWS) {
        hipLaunchKernelGGL(evg_dqn_delta_kernel<true>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, g);
    } else {
        long long blocks = (rows + 63) / 64;
        if (blocks > EVG_DQN_GRAD_MAX_BLOCKS) blocks = EVG_DQN_GRAD_MAX_BLOCKS;
        hipLaunchKernelGGL(evg_dqn_delta_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, g);
    }
    hipLaunchKernelGGL(evg_dqn_wgrad_kernel, dim3((unsigned)(g.CG * g.S)), dim3(256), 0, s, g);
    if (g.S > 1) {
        const int total = DQ_OUT * net.h1 + net.h1 * DQ_IN + DQ_OUT + net.h1;
        hipLaunchKernelGGL(evg_dqn_grad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g);
    }
    return (int)hipGetLastError();
}
