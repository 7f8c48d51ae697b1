// replay_priority_kernels.inc -- prioritized sampling for the Smart_State replay memory (include/evg.h, evg_replay_priority: agents/DQN/PrioritizedMemory.py
// over the ring of replay_kernels.inc).  Included by evg_kernels.hip after replay_kernels.inc (namespace evg); evg_replay_gather_kernel writes the batch.
//
//   evg_prio_clear_kernel     zeroes the plane, wmax = 1.0f
//   evg_prio_update_kernel    one thread per handle, launched twice: phase 0 resets (stale record: seven zeros + the stamp; else 0.0f at entry k),
//                             phase 1 takes the maximum (atomicMax on the bits of w at entry k and on wmax) -- no result depends on thread order
//   evg_prio_scan_kernel      per-record sums of the integer weights q -> per-4-record exclusive prefix inside each 1 024-record block, block sums of
//                             q and of the transition counts
//   evg_prio_top_kernel       one workgroup: exclusive prefix of the block sums, Q, the transition count, the sample call index
//   evg_prio_draw_kernel      one thread per draw: t = umul64hi(u, Q) -> (slot, env, seat, row) by two searches and a walk; its q, the batch's least q
//   evg_prio_weights_kernel   one thread per draw: (T q / Q) ** -beta over the batch's largest, in float64, rounded once

// evg_replay_priority as the kernels take it (the launchers copy the descriptor's fields)
struct PrioArgs {
    float alpha;
    float* plane;
    unsigned long long* pscan;
    unsigned long long* pctl;
};

constexpr int RP_PDRAW_DOMAIN = 7;         // Philox counter word 3 of the prioritized draws (the uniform ones use RP_DRAW_DOMAIN)

// the stamp of the record a plane row belongs to, from the record's meta {turn, episode, ...}
__device__ __forceinline__ uint32_t rp_stamp(const int4 meta) { return 0x80000000u | (((uint32_t)meta.y & 0x7FFFFFu) << 8) | ((uint32_t)meta.x & 0xFFu); }

// q of a weight: floor(w * 2^(32 - e)) with frexp(wmax) = (m, e), at least 1 (w <= wmax gives q < 2^32)
__device__ __forceinline__ unsigned long long rp_q(float w, int shift) {
    const unsigned long long q = (unsigned long long)ldexp((double)w, shift);
    return q ? q : 1ull;
}

__device__ __forceinline__ int rp_qshift(float wmax) {
    int e;
    (void)frexp((double)wmax, &e);
    return 32 - e;
}

// the integer weights of record r's `c` transitions (c = its count, 1..7): a stored weight where the row's stamp is the record's and the entry was
// updated, wmax otherwise
__device__ __forceinline__ void rp_record_q(const evg_replay& m, const float* __restrict__ plane, long long r, int c, float wmax, int shift,
                                            unsigned long long (&q)[NA]) {
    const float4 a = reinterpret_cast<const float4*>(plane)[2 * r], b = reinterpret_cast<const float4*>(plane)[2 * r + 1];
    const bool fresh = __float_as_uint(b.w) == rp_stamp(reinterpret_cast<const int4*>(m.meta)[r]);
    const float w[NA] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
#pragma unroll
    for (int k = 0; k < NA; ++k) q[k] = k < c ? rp_q(fresh && w[k] != 0.0f ? w[k] : wmax, shift) : 0ull;
}

__global__ void __launch_bounds__(256) evg_prio_clear_kernel(PrioArgs p, long long R) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // one float4 = half a plane row
    if (i < 2 * R) reinterpret_cast<float4*>(p.plane)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < 4) p.pctl[i] = i == 0 ? (unsigned long long)__float_as_uint(1.0f) : 0ull;
}

__global__ void __launch_bounds__(256) evg_prio_update_kernel(evg_replay m, PrioArgs p, int N, int batch, const int4* __restrict__ handles,
                                                              const float* __restrict__ priorities, int phase) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    const int4 h = handles[i];
    const float pr = priorities[i];
    const int S = m.num_seats;
    int ok = h.x >= 0 && h.x < m.slots && h.y >= 0 && h.y < N && h.z >= 0 && h.z < S && h.w >= 0 && h.w < NA;
    long long rec = 0;
    uint32_t rows = 0;
    if (ok) {
        const long long es = (long long)h.y * S + h.z;
        rec = (long long)h.x * N * S + es;
        rows = rp_row_mask(rp_dirs(m, N, h.x, es));
        ok = m.count[rec] != 0 && ((rows >> h.w) & 1u);
    }
    const bool good = pr > 0.0f && pr <= 3.402823466e+38f;                     // not NaN, not infinite, not <= 0
    if (phase == 0) {
        if (!ok) atomicOr(&m.ctl[1], (unsigned long long)EVG_REPLAY_S_BAD_HANDLE);
        if (!good) atomicOr(&m.ctl[1], (unsigned long long)EVG_REPLAY_S_BAD_PRIORITY);
    }
    if (!ok || !good) return;
    const int k = __popc(rows & ((1u << h.w) - 1u));                           // the row's rank among the record's transitions
    float* row = p.plane + 8 * rec;
    if (phase == 0) {
        const uint32_t stamp = rp_stamp(reinterpret_cast<const int4*>(m.meta)[rec]);
        if (__float_as_uint(row[7]) != stamp) {                                // a previous occupant's weights: every racing store writes these values
            reinterpret_cast<float4*>(row)[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            reinterpret_cast<float4*>(row)[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(stamp));
        } else {
            row[k] = 0.0f;
        }
        return;
    }
    float w = p.alpha == 1.0f ? pr : (p.alpha == 0.0f ? 1.0f : (float)pow((double)pr, (double)p.alpha));
    if (w < 1.17549435e-38f) w = 1.17549435e-38f;                              // FLT_MIN: a stored weight is never 0 ("never updated") or subnormal
    const uint32_t bits = __float_as_uint(w);                                  // positive floats order as their bits
    atomicMax(reinterpret_cast<unsigned int*>(row) + k, bits);
    atomicMax(&p.pctl[0], (unsigned long long)bits);
}

// exclusive prefix of 64-bit values over a 256-thread workgroup; the block's total in *total
__device__ __forceinline__ unsigned long long rp_block_exclusive64(unsigned long long v, unsigned long long* lds, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    unsigned long long base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    *total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + x - v;
}

// pscan layout: [G] group prefixes, [nb] block sums of q (then their exclusive prefix), [nb] block sums of the counts
__global__ void __launch_bounds__(256) evg_prio_scan_kernel(evg_replay m, PrioArgs p, long long R) {
    __shared__ unsigned long long lds[4];
    __shared__ int ldc[4];
    const float wmax = __uint_as_float((uint32_t)p.pctl[0]);
    const int shift = rp_qshift(wmax);
    const long long r0 = (long long)blockIdx.x * RP_SCAN_BLOCK + 4 * threadIdx.x;
    unsigned long long v = 0;
    int cnt = 0;
    for (int j = 0; j < 4; ++j) {
        const long long r = r0 + j;
        const int c = r < R ? (int)m.count[r] : 0;
        if (c) {
            unsigned long long q[NA];
            rp_record_q(m, p.plane, r, c < NA ? c : NA, wmax, shift, q);
#pragma unroll
            for (int k = 0; k < NA; ++k) v += q[k];
            cnt += c;
        }
    }
    unsigned long long total;
    const unsigned long long ex = rp_block_exclusive64(v, lds, &total);
    int ctotal;
    (void)rp_block_exclusive(cnt, ldc, &ctotal);
    const long long g = r0 / 4, G = (R + 3) / 4;
    const long long nb = (R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK;
    if (g < G) p.pscan[g] = ex;
    if (threadIdx.x == 0) {
        p.pscan[G + blockIdx.x] = total;
        p.pscan[G + nb + blockIdx.x] = (unsigned long long)ctotal;
    }
}

// one workgroup: block sums of q -> exclusive block prefix (in place), Q -> pctl[1]; the transition count -> ctl[2]; the call index of this sample ->
// ctl[3], ctl[0] + 1 -> ctl[0] (the counter evg_replay_sample advances); the batch's least q starts at its identity
__global__ void __launch_bounds__(256) evg_prio_top_kernel(evg_replay m, PrioArgs p, long long R) {
    __shared__ unsigned long long lds[4];
    const long long G = (R + 3) / 4;
    const int nb = (int)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK);
    unsigned long long* bs = p.pscan + G;
    const unsigned long long* bc = bs + nb;
    const int per = (nb + 255) / 256;
    const int lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    unsigned long long v = 0, c = 0;
    for (int b = lo; b < hi; ++b) {
        v += bs[b];
        c += bc[b];
    }
    unsigned long long total, ctotal;
    unsigned long long run = rp_block_exclusive64(v, lds, &total);
    (void)rp_block_exclusive64(c, lds, &ctotal);
    for (int b = lo; b < hi; ++b) {
        const unsigned long long x = bs[b];
        bs[b] = run;
        run += x;
    }
    if (threadIdx.x == 0) {
        p.pctl[1] = total;
        p.pctl[2] = ~0ull;
        m.ctl[2] = ctotal;
        m.ctl[3] = m.ctl[0];
        m.ctl[0] = m.ctl[0] + 1ull;
        if (ctotal == 0ull) m.ctl[1] |= (unsigned long long)EVG_REPLAY_S_EMPTY;
    }
}

// last index i in [lo, hi) with a[i] <= t (a non-decreasing, a[lo] <= t)
__device__ __forceinline__ long long rp_search64(const unsigned long long* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) evg_prio_draw_kernel(evg_replay m, PrioArgs p, int N, long long R, int batch, uint32_t seed_lo,
                                                               uint32_t seed_hi, int4* __restrict__ handles, uint32_t* __restrict__ q_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    const unsigned long long T = m.ctl[2], call = m.ctl[3], Q = p.pctl[1];
    if (T == 0ull || Q == 0ull) {              // empty memory: an invalid handle, which the gather turns into zeros
        handles[i] = make_int4(-1, -1, -1, -1);
        q_out[i] = 0u;
        return;
    }
    const float wmax = __uint_as_float((uint32_t)p.pctl[0]);
    const int shift = rp_qshift(wmax);
    const uint4 w = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)RP_PDRAW_DOMAIN), seed_lo, seed_hi);
    const unsigned long long t = __umul64hi(((unsigned long long)w.x << 32) | (unsigned long long)w.y, Q);     // position in [0, Q)
    const long long G = (R + 3) / 4;
    const long long nb = (R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK;
    const long long b = rp_search64(p.pscan + G, 0, nb, t);
    const unsigned long long tb = t - p.pscan[G + b];
    const long long g0 = b * (RP_SCAN_BLOCK / 4), g1 = g0 + RP_SCAN_BLOCK / 4 < G ? g0 + RP_SCAN_BLOCK / 4 : G;
    const long long g = rp_search64(p.pscan, g0, g1, tb);
    unsigned long long k = tb - p.pscan[g];
    // walk the group's (up to four) records; position k falls into one of their transitions
    long long rec = -1;
    int rank = 0;
    unsigned long long qsel = 0;
    bool found = false;
    for (int j = 0; j < 4; ++j) {
        const long long r = 4 * g + j;
        const int c = r < R ? (int)m.count[r] : 0;
        if (!c || found) continue;
        unsigned long long q[NA];
        rp_record_q(m, p.plane, r, c < NA ? c : NA, wmax, shift, q);
#pragma unroll
        for (int x = 0; x < NA; ++x) {
            if (x < c && !found) {
                rec = r;
                rank = x;
                qsel = q[x];
                if (k < q[x]) found = true;
                else k -= q[x];
            }
        }
    }
    if (rec < 0) {                             // (a group without a counted record holds no position)
        handles[i] = make_int4(-1, -1, -1, -1);
        q_out[i] = 0u;
        return;
    }
    const int S = m.num_seats;
    const long long plane = (long long)N * S;
    const int slot = (int)(rec / plane);
    const long long es = rec - (long long)slot * plane;
    uint32_t rows = rp_row_mask(rp_dirs(m, N, slot, es));
    for (int j = 0; j < rank; ++j) rows &= rows - 1u;                          // the rank-th counted row
    handles[i] = make_int4(slot, (int)(es / S), (int)(es % S), rows ? (int)__builtin_ctz(rows) : -1);
    q_out[i] = (uint32_t)qsel;
    atomicMin(&p.pctl[2], qsel);
}

// weights[i] holds draw i's q (pdraw); the batch's largest importance weight belongs to its least q (beta >= 0)
__global__ void __launch_bounds__(256) evg_prio_weights_kernel(evg_replay m, PrioArgs p, int batch, float beta, float* __restrict__ weights) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    const uint32_t q = reinterpret_cast<const uint32_t*>(weights)[i];
    const unsigned long long T = m.ctl[2], Q = p.pctl[1], qmin = p.pctl[2];
    float out = 0.0f;
    if (q != 0u && T != 0ull && Q != 0ull) {
        const double t = (double)T, total = (double)Q, nb = -(double)beta;
        out = (float)(pow(t * (double)q / total, nb) / pow(t * (double)qmin / total, nb));
    }
    weights[i] = out;
}

static inline PrioArgs prio_args(const evg_replay_priority& p) { return PrioArgs{p.alpha, p.plane, p.pscan, p.pctl}; }

int launch_replay_priority_clear(const DevState& S, const evg_replay& m, const evg_replay_priority& p, void* stream) {
    const long long R = (long long)m.slots * S.N * m.num_seats;
    hipLaunchKernelGGL(evg_prio_clear_kernel, dim3((unsigned)((2 * R + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), prio_args(p), R);
    return (int)hipGetLastError();
}

int launch_replay_priority_update(const DevState& S, const evg_replay& m, const evg_replay_priority& p, int batch, const int32_t* handles,
                                  const float* priorities, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const PrioArgs a = prio_args(p);
    for (int phase = 0; phase < 2; ++phase)
        hipLaunchKernelGGL(evg_prio_update_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, m, a, S.N, batch,
                           reinterpret_cast<const int4*>(handles), priorities, phase);
    return (int)hipGetLastError();
}

int launch_replay_priority_draw(const DevState& S, const evg_replay& m, const evg_replay_priority& p, int batch, uint64_t seed, float beta, int32_t* handles,
                                float* weights, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long R = (long long)m.slots * S.N * m.num_seats;
    const unsigned grid = (unsigned)((batch + 255) / 256);
    const PrioArgs a = prio_args(p);
    hipLaunchKernelGGL(evg_prio_scan_kernel, dim3((unsigned)((R + RP_SCAN_BLOCK - 1) / RP_SCAN_BLOCK)), dim3(256), 0, s, m, a, R);
    hipLaunchKernelGGL(evg_prio_top_kernel, dim3(1), dim3(256), 0, s, m, a, R);
    hipLaunchKernelGGL(evg_prio_draw_kernel, dim3(grid), dim3(256), 0, s, m, a, S.N, R, batch, (uint32_t)seed, (uint32_t)(seed >> 32),
                       reinterpret_cast<int4*>(handles), reinterpret_cast<uint32_t*>(weights));
    hipLaunchKernelGGL(evg_prio_weights_kernel, dim3(grid), dim3(256), 0, s, m, a, batch, beta, weights);
    return (int)hipGetLastError();
}
