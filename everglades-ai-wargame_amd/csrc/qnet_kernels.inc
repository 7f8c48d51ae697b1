// qnet_kernels.inc -- the Smart_State Q network's forward pass (include/evg.h, evg_smart_qnet): agents/Smart_State/QNetwork.py, inference only.
// Included by evg_kernels.hip (namespace evg).
//
//   evg_qnet_kernel<EXPANDED>   256 threads = 4 wavefronts; a wavefront owns 16 rows at a time (16 envs of one seat and one swarm index in the compact
//                               layouts, 16 rows of x in the expanded one) and runs all three layers on them with v_mfma_f32_16x16x4_f32
//
// Numerics.  v_mfma_f32_16x16x4_f32 computes D[i][j] = fma(A[i][3] B[3][j], fma(A[i][2] B[2][j], fma(A[i][1] B[1][j], fma(A[i][0] B[0][j], C[i][j]))))
// exactly (one rounding per product, k ascending), so a sequence of them over k-steps 0, 1, 2, ... with C = the bias IS the chain of the contract.
// The operands are always taken in natural k order (the hidden tiles go through LDS, never accumulator-as-operand), and every padded k position has a
// zero weight and a zero input, which leaves the chain unchanged.  The zero input is enforced, not incidental: the ReLU is torch's (x < 0 ? 0 : x, a NaN
// stays a NaN, on the hidden layers and on the output), so a padded hidden unit -- whose accumulator is 0 + sum of x * 0, NaN for an Inf or NaN x -- is
// an exact zero in the tile (zeroed once, never stored to: qn_store_col); otherwise NaN * 0 would poison every output of a row that has one non-finite input.  The compact layouts run the chain prefix b1 + shared[0..33] once per 16 envs and
// continue it per swarm with swarm[s][0..12] (W1 columns 34..46), then add W1[j][47 + s] on the VALU: the one-hot term.
//
// Lane maps (16x16x4 f32): A lane l = X[row l & 15][k l >> 4], B lane l = W[column l & 15][k l >> 4], C/D lane l register r = [row 4 (l >> 4) + r]
// [column l & 15].  The weights live in registers as B fragments (staged through LDS once per workgroup), the rows' inputs are read as A fragments
// straight from HBM, the hidden tiles are written to a per-wavefront LDS tile in the D layout and read back in the A layout.

constexpr int QN_IN = 59, QN_OUT = 5, QN_H = 64;       // input width, output width, the largest hidden size
constexpr int QN_WAVES = 4;                            // wavefronts per workgroup
constexpr int QN_HS = 68;                              // row stride of a hidden tile in LDS (68 = 4 mod 64: the A-layout read is conflict-free; the 4 spare columns take the padded units)
constexpr int QN_W1S = 61, QN_W2S = 65, QN_W3S = 65;   // row strides of the staged weights (odd: the B-fragment reads spread over the banks)
constexpr int QN_STAGE = QN_H * QN_W1S + QN_H * QN_W2S + 16 * QN_W3S;   // staged weights (floats)
constexpr int QN_WAVE_LDS = 2 * 16 * QN_HS + 16 * 60;                    // per wavefront: two hidden tiles and the 16 x 60 Q tile
constexpr int QN_UNION = QN_STAGE > QN_WAVES * QN_WAVE_LDS ? QN_STAGE : QN_WAVES * QN_WAVE_LDS;
constexpr int QN_W1PS = 37;                             // row stride of the staged shared columns W1[:, 0..35] (the compact prefix)
constexpr int QN_FIXED = 64 + 64 + 16 + 12 * 64 + QN_H * QN_W1PS;   // b1, b2, b3, the one-hot columns W1[:, 47 + s], W1[:, 0..35]

typedef float qn_f4 __attribute__((ext_vector_type(4)));

struct QnetSet {
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* w3;
    const float* b3;
};

struct QnetArgs {
    QnetSet set[2];
    int h1, h2, final_relu, num_seats;     // num_seats: the S of the compact layouts (1 or 2); 1 for the expanded one
    long long rows;
    const float* in0;
    const float* in1;
    float* out;
};

__device__ __forceinline__ qn_f4 qn_mfma(float a, float b, qn_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ void qn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// torch.relu: a NaN stays a NaN (fmaxf would drop it); the sign of a zero result is not part of the contract.  IEEE 754-2019 maximum, which gfx950 has
// as one instruction (v_maximum3_f32), so the ReLU costs what fmaxf cost
__device__ __forceinline__ float qn_relu(float x) { return __builtin_elementwise_maximum(x, 0.0f); }

// The column of a hidden tile that unit 16 t + col of a layer of hn units is stored to: its own -- or, for a padded unit (>= hn), one of the row's four
// spare columns (the row stride is 64 + 4), which nothing reads.  A padded unit's accumulator is 0 + sum of x * 0, a NaN as soon as an x is Inf or NaN,
// which the next layer's zero weight would not take out (NaN * 0); stored aside, it leaves the padded columns with the exact zeros that qn_zero_tile
// wrote once, before the wavefront's first group.  Lane-constant, computed before the loop over the groups: the stores stay unconditional.
__device__ __forceinline__ int qn_store_col(int t, int col, int hn, int width) { return 16 * t + col < hn ? 16 * t + col : width + (col & 3); }

// acc (D layout) -> relu -> hidden tile in LDS, tile t to column cols[t] (qn_store_col)
__device__ __forceinline__ void qn_store_hidden(float* __restrict__ tile, const qn_f4 (&acc)[4], const int (&cols)[4], int lane) {
    const int row0 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(row0 + r) * QN_HS + cols[t]] = qn_relu(acc[t][r]);
}

// a wavefront's n floats of LDS <- exact zeros (the padded columns of its hidden tiles are never written again)
__device__ __forceinline__ void qn_zero_tile(float* __restrict__ tile, int n, int lane) {
    for (int i = lane; i < n; i += 64) tile[i] = 0.0f;
}

// Layers 2 and 3 of 16 rows whose first hidden layer (after the ReLU) is in tile h1t: returns the Q tile (D layout; columns 0..4 are Q)
__device__ __forceinline__ qn_f4 qn_layers23(const float* __restrict__ h1t, float* __restrict__ h2t, const float (&w2f)[16][4], const float (&w3f)[16],
                                            const float (&b2v)[4], float b3v, int n2, const int (&cols2)[4], int final_relu, int lane) {
    const int arow = (lane & 15) * QN_HS + (lane >> 4);
    qn_f4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = qn_f4{b2v[t], b2v[t], b2v[t], b2v[t]};
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        if (st < n2) {
            const float a = h1t[arow + 4 * st];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = qn_mfma(a, w2f[st][t], acc[t]);
        }
    }
    qn_store_hidden(h2t, acc, cols2, lane);
    qn_wave_sync();
    qn_f4 q = qn_f4{b3v, b3v, b3v, b3v};
#pragma unroll
    for (int st = 0; st < 16; ++st) q = qn_mfma(h2t[arow + 4 * st], w3f[st], q);   // (k >= h2: zero weight, zero input)
    if (final_relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = qn_relu(q[r]);
    return q;
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_qnet_kernel(QnetArgs a) {
    __shared__ float fixed[QN_FIXED];
    __shared__ __attribute__((aligned(16))) float lds[QN_UNION];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = blockIdx.y;
    const QnetSet W = a.set[seat];
#define QN_GROUPED 0
#include "qnet_body.inc"
#undef QN_GROUPED
}

int launch_smart_qnet(const evg_qnet& net, int layout, long long rows, const float* in0, const float* in1, float* q_out, int num_cu, void* stream) {
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
    // persistent-style grid: two workgroups per CU are resident (the weight registers allow 2 wavefronts per SIMD); each wavefront loops over its groups
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_qnet_kernel<true>, dim3((unsigned)blocks, 1), dim3(64 * QN_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(evg_qnet_kernel<false>, dim3((unsigned)blocks, (unsigned)a.num_seats), dim3(64 * QN_WAVES), 0, s, a);
    return (int)hipGetLastError();
}
