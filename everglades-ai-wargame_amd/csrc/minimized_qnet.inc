// minimized_qnet.inc -- the Minimized agents' Q network's forward pass (include/evg.h, evg_minimized_qnet): agents/Minimized/QNetwork.py, inference only:
// relu(fc2(relu(fc1(x)))), 59 -> h1 -> 11 with h1 in 1..128 (80 by default, carried in the agents' pickles).  Included by evg_kernels.hip (namespace evg),
// after qnet_kernels.inc, whose helpers (qn_f4, qn_mfma, qn_wave_sync) and numeric contract it shares:
//
//   evg_mini_qnet_kernel<EXPANDED>   (its body: minimized_qnet_body.inc, shared with the grouped kernel of population_kernels.inc)
//                                    256 threads = 4 wavefronts; a wavefront owns 16 rows at a time (16 envs of one seat in the compact layouts, 16 rows of
//                                    x in the expanded one) and runs both layers on them with v_mfma_f32_16x16x4_f32
//
// Numerics: as qnet_kernels.inc -- a sequence of 16x16x4 MFMAs over k-steps 0, 1, 2, ... with C = the bias IS the chain acc = b[j], fmaf(W[j][k], x[k], acc)
// for k ascending; operands in natural k order, padded k positions with zero weight and zero input; the compact layouts run the 34-term shared prefix once
// per 16 envs and add the one-hot term W1[j][47 + s] on the VALU.  The ReLU is torch's (a NaN stays a NaN, hidden layer and output), and the padded
// hidden units inside the last tile (index >= h1) are exact zeros whatever their accumulator holds (0 + sum of x * 0 is NaN for a non-finite x): zeroed once, never stored to.
//
// Hidden up to 128 is up to 8 column tiles of 16; the 11 outputs are one tile.  Tiles beyond the network's h1 are skipped (wave-uniform branches), so a
// network of 80 runs 5.  Registers hold what every group of rows reuses and fits: the 13 swarm columns of W1 (compact; 4 k-steps x 8 tiles), W2 (32 k-steps)
// and the biases.  The layer-1 fragments that do not fit next to them -- all 15 k-steps x 8 tiles of the expanded layout, the 9 x 8 of the compact prefix
// -- are read from LDS at every use, where the whole workgroup shares one zero-padded copy.  The hidden tile goes through a per-wavefront LDS tile (D layout
// in, A layout out); Q leaves the accumulator straight to HBM: a row's 11 values are 44 contiguous bytes.

constexpr int MQ_OUT = 11, MQ_H = 128, MQ_TILES = MQ_H / 16;   // output width, the largest hidden size, its column tiles
constexpr int MQ_HS = 132;                                     // row stride of the hidden tile in LDS (132 = 4 mod 64: the A-layout read is conflict-free; 4 spare columns)
constexpr int MQ_W1S = 61, MQ_W1PS = 37;                       // row strides of the staged W1 (expanded: 60 columns) and of its shared columns (compact: 36)
constexpr int MQ_KX = 15, MQ_KP = 9, MQ_KS = 4, MQ_K2 = MQ_H / 4;   // k-steps: expanded layer 1, compact prefix, swarm columns, layer 2

struct MiniQnetSet {
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
};

struct MiniQnetArgs {
    MiniQnetSet set[2];
    int h1, final_relu, num_seats;     // num_seats: the S of the compact layouts (1 or 2); 1 for the expanded one
    long long rows;
    const float* in0;
    const float* in1;
    float* out;
};

// layer 2 of 16 rows whose hidden layer (after the ReLU) is in tile ht: the Q tile (D layout; columns 0..10 are Q)
// (k runs over the nt column tiles layer 1 wrote: k >= h1 inside the last tile has a zero weight and an exact zero input: qn_store_col)
__device__ __forceinline__ qn_f4 mq_layer2(const float* __restrict__ ht, const float (&w2f)[MQ_K2], float b2v, int nt, int final_relu, int lane) {
    const int arow = (lane & 15) * MQ_HS + (lane >> 4);
    qn_f4 q = qn_f4{b2v, b2v, b2v, b2v};
#pragma unroll
    for (int t = 0; t < MQ_TILES; ++t)
        if (t < nt)
#pragma unroll
            for (int st = 4 * t; st < 4 * t + 4; ++st) q = qn_mfma(ht[arow + 4 * st], w2f[st], q);
    if (final_relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = qn_relu(q[r]);
    return q;
}

// acc (D layout) of a column tile -> relu (qn_relu: a NaN stays) -> column c of the hidden tile (qn_store_col: the padded units of the last tile,
// >= h1, go to the row's spare columns 128..131, and theirs keep the exact zeros the tile was filled with before the wavefront's first group)
__device__ __forceinline__ void mq_store_hidden(float* __restrict__ ht, const qn_f4 acc, int c, int lane) {
    const int row0 = 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) ht[(row0 + r) * MQ_HS + c] = qn_relu(acc[r]);
}

// GROUPED form (population_kernels.inc): position i of the workgroup's member list names the row list[i] of the caller's tensors (clamped: a list is
// never trusted with an address; the grouped form has at most 2^24 rows)
__device__ __forceinline__ int mq_list_row(const int* __restrict__ list, long long i, long long rows) {
    const int r = list[i];
    return r < 0 ? 0 : (r < rows ? r : (int)rows - 1);
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_mini_qnet_kernel(MiniQnetArgs a) {
    // the workgroup's copy of the layer-1 weights that are read at every use: expanded W1[:, 0..59] (stride 61); compact W1[:, 0..35] (stride 37), then
    // the one-hot columns W1[:, 47 + s] as [12][128]
    constexpr int WLDS = EXPANDED ? MQ_H * MQ_W1S : MQ_H * MQ_W1PS + 12 * MQ_H;
    __shared__ float wl[WLDS];
    __shared__ float tiles[QN_WAVES][16 * MQ_HS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = blockIdx.y;
    const MiniQnetSet W = a.set[seat];
#define MQ_GROUPED 0
#include "minimized_qnet_body.inc"
#undef MQ_GROUPED
}

int launch_minimized_qnet(const evg_mini_qnet& net, int layout, long long rows, const float* in0, const float* in1, float* q_out, int num_cu, void* stream) {
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
    // persistent-style grid: two workgroups per CU are resident (LDS); each wavefront loops over its groups
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_mini_qnet_kernel<true>, dim3((unsigned)blocks, 1), dim3(64 * QN_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(evg_mini_qnet_kernel<false>, dim3((unsigned)blocks, (unsigned)a.num_seats), dim3(64 * QN_WAVES), 0, s, a);
    return (int)hipGetLastError();
}
