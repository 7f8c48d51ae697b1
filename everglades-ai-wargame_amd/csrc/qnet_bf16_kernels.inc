// qnet_bf16_kernels.inc -- the reduced-precision forward of the two Q networks (include/evg_qnet_bf16.h: evg_smart_qnet_bf16, evg_minimized_qnet_bf16),
// for acting and for the target network: every layer on v_mfma_f32_16x16x32_bf16.  Included by evg_kernels.hip (namespace evg) under EVG_BF16
// (`make bf16`, libevg_bf16.so), after qnet_kernels.inc and minimized_qnet.inc, whose argument structs (QnetArgs, MiniQnetArgs), qn_f4 and qn_relu it
// shares; the fp32 evaluators are not touched.
// The two kernels' bodies are qnet_bf16_body.inc and minimized_qnet_bf16_body.inc (QB_GROUPED 0): program text that the grouped kernels of
// population_bf16_kernels.inc include as well (QB_GROUPED 1).
//
//   evg_qnet_bf16_kernel<EXPANDED>        59 -> h1 -> h2 -> 5, h1, h2 in 1..64
//   evg_mini_qnet_bf16_kernel<EXPANDED>   59 -> h1 -> 11, h1 in 1..128
//   256 threads = 4 wavefronts; a wavefront owns 16 rows at a time (16 envs of one seat in the compact layouts, 16 rows of x in the expanded one)
//
// Numerics (the contract of include/evg_qnet_bf16.h): inputs and weights rounded to bf16 (RNE, v_cvt_pk_bf16_f32), biases fp32, exact products, fp32
// accumulation in the matrix core's own order, hidden activations bf16_rne(relu(pre)) with the NaN-keeping ReLU, the output layer the fp32
// pre-activation.  The one-hot term of the compact layouts is a product of the MFMA like any other: the swarm k-step carries an input of 1.0 at the
// swarm's own position and W1[j][47 + s] opposite it.
//
// Orientation.  Every product is  (layer output)^T = W . (layer input)^T :  the weights are the A operand (row = unit j), the 16 rows of the group are
// the 16 COLUMNS of B and of the result.  The C/D map of a 16x16 tile -- lane l register r = [row 4 (l >> 4) + r][column l & 15] -- then leaves a lane
// with 4 units of ITS OWN data row per tile, and the next layer sums over exactly that row index: the accumulators of two tiles, through the ReLU and
// v_cvt_pk_bf16_f32, ARE the next MFMA's B fragment, with no LDS round trip and no lane movement.  The B map is lane l element i = [k 8 (l >> 4) + i]
// [column l & 15]; fed with tiles 2u and 2u + 1, element i of lane quarter q holds unit 32 u + 16 (i >> 2) + 4 q + (i & 3), so the weights' A fragment
// (lane l element i = [row l & 15][k 8 (l >> 4) + i]) is staged with that same permutation of k (QB_CHAINED).  Layer 1 reads its inputs from memory
// and takes k in natural order (QB_NATURAL), or, for a swarm's 13 features and its one-hot position, four of each per lane quarter (QB_SWARM).
//
// Padding.  A fragment element whose unit or column does not exist is a zero weight.  A padded hidden unit (>= h1, >= h2) has the accumulator
// 0 + sum of x * 0, a NaN for a non-finite x, which the next layer's zero weight would not take out: it is replaced by an exact zero on its way into
// the B fragment (qb_pack).  Rows past the end of the batch enter as zero inputs and store nothing.
//
// The weights are read in place on every call: the workgroup converts them to bf16 into LDS, already in fragment order (16 bytes per lane and
// fragment: one ds_read_b128, conflict-free), and each wavefront keeps in registers the fragments that every swarm reuses.

typedef __bf16 qb_bf8 __attribute__((ext_vector_type(8)));

enum { QB_NATURAL = 0, QB_CHAINED = 1, QB_SWARM = 2 };

__device__ __forceinline__ qn_f4 qb_mfma(qb_bf8 a, qb_bf8 b, qn_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// The column of the weight matrix that element i of lane quarter q holds in k-step s of an A fragment (-1: none, a zero)
template <int KIND>
__device__ __forceinline__ int qb_src_col(int s, int q, int i) {
    if (KIND == QB_NATURAL) return 32 * s + 8 * q + i;
    if (KIND == QB_CHAINED) return 32 * s + 16 * (i >> 2) + 4 * q + (i & 3);
    const int f = 4 * q + (i & 3);                       // QB_SWARM: elements 0..3 swarm features 4 q .. 4 q + 3, elements 4..7 one-hot positions 4 q .. 4 q + 3
    return i < 4 ? (f < 13 ? 34 + f : -1) : (f < 12 ? 47 + f : -1);
}

// dst[(t * ksteps + s) * 64 + lane] <- the A fragment of tile t (units 16 t .. 16 t + 15 of w [nrows][ld]), k-step s: bf16_rne of the weights, zeros
// where the unit (>= nrows) or the column (>= kmax) does not exist
template <int KIND>
__device__ __forceinline__ void qb_stage(qb_bf8* __restrict__ dst, const float* __restrict__ w, int ld, int nrows, int kmax, int tiles, int ksteps, int tid) {
    for (int f = tid; f < tiles * ksteps * 64; f += 64 * QN_WAVES) {
        const int l = f & 63, ts = f >> 6, t = ts / ksteps, s = ts - t * ksteps;
        const int j = 16 * t + (l & 15), q = l >> 4;
        qb_bf8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = qb_src_col<KIND>(s, q, i);
            const bool have = j < nrows && k >= 0 && k < kmax;
            const float x = w[have ? j * ld + k : 0];     // (read without a branch, as the inputs are: qb_load8)
            v[i] = (__bf16)(have ? x : 0.0f);
        }
        dst[f] = v;
    }
}

// this lane's bias registers of tile t: units 16 t + 4 q + r (zeros past n)
__device__ __forceinline__ qn_f4 qb_bias(const float* __restrict__ b, int n, int t, int q) {
    qn_f4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 16 * t + 4 * q + r;
        const float x = b[j < n ? j : 0];
        v[r] = j < n ? x : 0.0f;
    }
    return v;
}

// two accumulator tiles (units 32 u + 16 (i >> 2) + 4 q + (i & 3)) -> relu -> exact zeros for the padded units (>= n) -> bf16: the B fragment of k-step u
__device__ __forceinline__ qb_bf8 qb_pack(const qn_f4 lo, const qn_f4 hi, int u, int q, int n) {
    qb_bf8 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = (__bf16)(32 * u + 4 * q + i < n ? qn_relu(lo[i]) : 0.0f);
        v[4 + i] = (__bf16)(32 * u + 16 + 4 * q + i < n ? qn_relu(hi[i]) : 0.0f);
    }
    return v;
}

// Inputs are read without a branch -- a lane whose row or feature does not exist reads a position that does (its row clamped to the last one, the
// feature to the row's first) and selects a zero afterwards -- so that the loads of a group are all in flight at once.
// 8 consecutive inputs row[k0 .. k0 + 7] of a row of kmax features -> bf16, zeros from feature kmax on and for a row past the end
__device__ __forceinline__ qb_bf8 qb_load8(const float* __restrict__ row, int k0, int kmax, bool valid) {
    qb_bf8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = k0 + i;
        const float x = row[k < kmax ? k : 0];
        v[i] = (__bf16)((valid && k < kmax) ? x : 0.0f);
    }
    return v;
}

// features 4 q .. 4 q + 3 of one swarm (13 floats at p) as bf16, zeros past the 13th and for a row past the end: elements 0..3 of the swarm's B fragment
typedef __bf16 qb_bf4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ qb_bf4 qb_load_swarm(const float* __restrict__ p, int q, bool valid) {
    qb_bf4 x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = 4 * q + i;
        const float v = p[k < 13 ? k : 0];
        x[i] = (__bf16)((valid && k < 13) ? v : 0.0f);
    }
    return x;
}

// the B fragment of swarm s: elements 0..3 = its features (qb_load_swarm), elements 4..7 = 1.0 at one-hot position s (positions 4 q .. 4 q + 3)
__device__ __forceinline__ qb_bf8 qb_swarm_frag(const qb_bf4 x, int s, int q) {
    qb_bf8 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = x[i];
        v[4 + i] = (__bf16)(4 * q + i == s ? 1.0f : 0.0f);
    }
    return v;
}

// this lane's four values of a Q tile (outputs 4 q .. 4 q + 3 of its row; o points at the first of them) -> memory: all four, or the OUT - 4 q that exist
typedef float qb_f4u __attribute__((ext_vector_type(4), aligned(4)));
template <int OUT>
__device__ __forceinline__ void qb_store_q(float* __restrict__ o, const qn_f4 v, int q, bool valid) {
    const int n = OUT - 4 * q;
    if (valid && n >= 4) {
        *reinterpret_cast<qb_f4u*>(o) = v;
    } else if (valid && n > 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r < n) o[r] = v[r];
    }
}

// ------------------------------------------------------------------------------------------------------------------ Smart_State: 59 -> h1 -> h2 -> 5
// layers 2 and 3 of 16 rows whose first-layer accumulators are acc: the Q tile (lane l register r = Q[row l & 15][4 (l >> 4) + r])
__device__ __forceinline__ qn_f4 qb_smart_tail(const qn_f4 (&acc)[4], const qb_bf8 (&w2f)[4][2], const qb_bf8 (&w3f)[2], const qn_f4 (&b2v)[4],
                                               const qn_f4 b3v, int H1, int H2, int final_relu, int q) {
    const qb_bf8 h0 = qb_pack(acc[0], acc[1], 0, q, H1), h1 = qb_pack(acc[2], acc[3], 1, q, H1);
    qn_f4 a2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) a2[m] = qb_mfma(w2f[m][1], h1, qb_mfma(w2f[m][0], h0, b2v[m]));
    const qb_bf8 g0 = qb_pack(a2[0], a2[1], 0, q, H2), g1 = qb_pack(a2[2], a2[3], 1, q, H2);
    qn_f4 out = qb_mfma(w3f[1], g1, qb_mfma(w3f[0], g0, b3v));
    if (final_relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = qn_relu(out[r]);
    return out;
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_qnet_bf16_kernel(QnetArgs a) {
    // A fragments in LDS: layer 1 (expanded: 4 tiles x 2 k-steps; compact: the same 8 for the 34 shared columns, then 4 for the swarm k-step), layer 2
    // (4 x 2), layer 3 (1 x 2)
    constexpr int L1F = EXPANDED ? 8 : 12;
    __shared__ qb_bf8 w1s[L1F * 64], w2s[8 * 64], w3s[2 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = blockIdx.y;
    const QnetSet W = a.set[seat];
#define QB_GROUPED 0
#include "qnet_bf16_body.inc"
#undef QB_GROUPED
}

int launch_smart_qnet_bf16(const evg_qnet& net, int layout, long long rows, const float* in0, const float* in1, float* q_out, int num_cu, void* stream) {
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
    // the fp32 launch's grid: at most two workgroups per CU, each wavefront loops over its groups of 16 rows
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_qnet_bf16_kernel<true>, dim3((unsigned)blocks, 1), dim3(64 * QN_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(evg_qnet_bf16_kernel<false>, dim3((unsigned)blocks, (unsigned)a.num_seats), dim3(64 * QN_WAVES), 0, s, a);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ Minimized: 59 -> h1 -> 11
// the hidden layer's accumulators (tiles >= nt are not computed: zeros) -> the Q tile (lane l register r = Q[row l & 15][4 (l >> 4) + r])
__device__ __forceinline__ qn_f4 qb_mini_tail(const qn_f4 (&acc)[MQ_TILES], const qb_bf8 (&w2f)[MQ_TILES / 2], const qn_f4 b2v, int H1, int nt,
                                              int final_relu, int q) {
    qn_f4 out = b2v;
#pragma unroll
    for (int u = 0; u < MQ_TILES / 2; ++u)
        if (2 * u < nt) out = qb_mfma(w2f[u], qb_pack(acc[2 * u], acc[2 * u + 1], u, q, H1), out);      // (tile 2 u + 1 >= nt: every unit >= h1, zeros)
    if (final_relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = qn_relu(out[r]);
    return out;
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES, 2) evg_mini_qnet_bf16_kernel(MiniQnetArgs a) {     // (2 wavefronts per SIMD: at most 256 registers)
    // A fragments in LDS: layer 1 (expanded: 8 tiles x 2 k-steps; compact: the same 16 for the 34 shared columns, then 8 for the swarm k-step), layer 2
    // (1 tile x 4 k-steps); b1 zero-padded to 128
    constexpr int L1F = EXPANDED ? 2 * MQ_TILES : 3 * MQ_TILES;
    __shared__ qb_bf8 w1s[L1F * 64], w2s[(MQ_TILES / 2) * 64];
    __shared__ __attribute__((aligned(16))) float b1s[MQ_H];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = blockIdx.y;
    const MiniQnetSet W = a.set[seat];
#define QB_GROUPED 0
#include "minimized_qnet_bf16_body.inc"
#undef QB_GROUPED
}

int launch_minimized_qnet_bf16(const evg_mini_qnet& net, int layout, long long rows, const float* in0, const float* in1, float* q_out, int num_cu,
                               void* stream) {
    MiniQnetArgs a;
    for (int p = 0; p < 2; ++p) {
        const int q = p < net.num_sets ? p : 0;
        a.set[p] = MiniQnetSet{net.w1[q], net.b1[q], net.w2[q], net.b2[q]};
    }
    a.h1 = net.h1;
    a.final_relu = net.final_relu;
    a.num_seats = layout == EVG_QNET_COMPACT_SEATS ? 2 : 1;
    a.rows = rows;
    a.in0 = in0;
    a.in1 = in1;
    a.out = q_out;
    // the fp32 launch's grid: at most two workgroups per CU, each wavefront loops over its groups of 16 rows
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_mini_qnet_bf16_kernel<true>, dim3((unsigned)blocks, 1), dim3(64 * QN_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(evg_mini_qnet_bf16_kernel<false>, dim3((unsigned)blocks, (unsigned)a.num_seats), dim3(64 * QN_WAVES), 0, s, a);
    return (int)hipGetLastError();
}
