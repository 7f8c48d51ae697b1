// qnet_grad_kernels.inc -- the backward pass of the two Q networks' expanded fp32 forward (include/evg_qnet_grad.h: evg_smart_qnet_backward,
// evg_minimized_qnet_backward): the parameter gradients of optimize_model's policy forward.  Included by evg_kernels.hip (namespace evg) under EVG_GRAD
// (`make grad`, libevg_grad.so), after qnet_kernels.inc and minimized_qnet.inc, whose argument sets, lane maps and layer functions (qn_mfma,
// qn_store_hidden, qn_layers23, mq_store_hidden, mq_layer2) it uses: the forward chain of layers 2 and 3 is the forward's own code, and layer 1 is its
// fifteen k-steps with the bias as C.  The forward's kernel bodies (qnet_body.inc, minimized_qnet_body.inc) are not included: their LDS is a union of the
// staged weights and the wavefronts' tiles, and the backward needs W2 and W3 in LDS for as long as it runs.
//
//   evg_qnet_grad_kernel        59 -> h1 -> h2 -> 5   256 threads = 4 wavefronts, one wavefront per SIMD (up to 512 registers each)
//   evg_mini_qnet_grad_kernel   59 -> h1 -> 11
//   evg_qnet_grad_reduce_kernel the workgroups' partials -> the gradient tensors, in ascending workgroup order, with the optional clamp
// The two kernels' bodies are qnet_grad_body.inc and minimized_qnet_grad_body.inc (QG_GROUPED 0), shared with the grouped kernels of pop_learn_kernels.inc.
//
// A wavefront loops over groups of 16 rows.  For a group it recomputes a1, a2, q (tiles in LDS, q in the D layout), forms the deltas and adds the
// group's outer products into accumulator tiles that live in registers for the whole launch.
//
// Tile maps (v_mfma_f32_16x16x4_f32: A lane l = A[l & 15][l >> 4], B lane l = B[l >> 4][l & 15], D lane l register r = D[4 (l >> 4) + r][l & 15]).
//   outer products   gW[j][i] = sum over rows of d[row][j] a[row][i]: the row index is the MFMA's k.  The contract leaves the order of that sum open,
//                    so k-step st of lane quarter kq is taken to be row 4 kq + st: then register st of a delta tile in the D layout (rows 4 kq + r,
//                    unit l & 15) IS the A fragment of d^T for k-step st, with no transpose; the B fragment is a[4 kq + st][16 t + (l & 15)], read
//                    from the activation tile in LDS (row stride = 4 mod 64: the four quarters fall on disjoint banks), or from memory for x.
//   W^T d            d_prev[row][i] = sum_j d[row][j] W[j][i]: d goes through LDS into the A layout (as the forward's hidden tiles do), W[j][i] is
//                    read from LDS as B[k = j][n = i] (row stride 80 = 16 mod 64: conflict-free).
// The masks are a > 0 on the activation tile itself (Smart_State), or bits kept from the layer-1 accumulators (Minimized, whose one tile is reused for
// d2); a padded unit's activation is the exact zero of the forward's tile, so its mask is 0 and its delta an exact zero (a select, not a product).
//
// End of the launch: the four wavefronts' accumulators go through LDS, are summed in wavefront order, and the sum is the workgroup's partial in the
// caller's workspace (padded shapes: EVG_*_QNET_GRAD_PARTIAL floats).  No atomics anywhere: the order of every sum is a function of the grid alone.

constexpr int QG_W2S = 80;                              // row stride of W2 / W3 in LDS as B[k = unit out][n = unit in]
constexpr int QG_DS = 20;                               // row stride of the d3 tile (20: the A-layout read is conflict-free)
constexpr int QG_WAVE_LDS = 2 * 16 * QN_HS + 16 * QG_DS;   // per wavefront: the two hidden tiles and the d3 tile
constexpr int QG_LDS = 64 * QG_W2S + 8 * QG_W2S + QN_WAVES * QG_WAVE_LDS;
constexpr int QG_CHUNK = 3072;                          // floats of the partial that the four wavefronts sum at a time (48 rows of 64)
constexpr int QG_P = EVG_SMART_QNET_GRAD_PARTIAL, MG_P = EVG_MINI_QNET_GRAD_PARTIAL;
constexpr int MG_CHUNK = 2048;                          // 32 rows of gW1, or all of gW2 [16][128]
static_assert(QN_WAVES * QG_CHUNK <= QG_LDS && 3 * QG_CHUNK + 144 == QG_P, "the Smart_State partial is three chunks and the biases");
static_assert(5 * MG_CHUNK + 144 == MG_P, "the Minimized partial is five chunks and the biases");

struct QnetGradArgs {
    QnetSet W;
    int h1, h2, final_relu;
    long long rows;
    const float* x;
    const float* gq;
    float* partial;
};

__device__ __forceinline__ float qg_sum4(const qn_f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

__global__ void __launch_bounds__(64 * QN_WAVES) evg_qnet_grad_kernel(QnetGradArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[QG_LDS];
    const QnetSet W = a.W;
#define QG_GROUPED 0
#include "qnet_grad_body.inc"
#undef QG_GROUPED
}

// ------------------------------------------------------------------------------------------------------------------ Minimized: 59 -> h1 -> 11
struct MiniQnetGradArgs {
    MiniQnetSet W;
    int h1, final_relu;
    long long rows;
    const float* x;
    const float* gq;
    float* partial;
};

__global__ void __launch_bounds__(64 * QN_WAVES) evg_mini_qnet_grad_kernel(MiniQnetGradArgs a) {
    // the workgroup's zero-padded copy of W1[:, 0..59] (stride 61), read at every use as in the forward; the wavefronts' hidden tiles
    __shared__ __attribute__((aligned(16))) float lds[MQ_H * MQ_W1S + QN_WAVES * 16 * MQ_HS];
    static_assert(QN_WAVES * MG_CHUNK <= MQ_H * MQ_W1S + QN_WAVES * 16 * MQ_HS, "the staging of a chunk fits the LDS");
    const MiniQnetSet W = a.W;
#define QG_GROUPED 0
#include "minimized_qnet_grad_body.inc"
#undef QG_GROUPED
}

// ------------------------------------------------------------------------------------------------------------------ the reduction
// One thread per element of the gradient tensors (the nn.Linear shapes: nothing outside them is written): the sum of that element over the workgroups'
// partials in ascending workgroup order, the optional clamp, one store.
struct QnetGradSeg {
    float* dst;                                         // [rows][cols], contiguous
    int rows, cols, src, ld;                            // element [j][i] is partial[src + j * ld + i]
};

struct QnetGradReduceArgs {
    QnetGradSeg seg[6];
    int nseg, blocks, stride, total;                    // partials, floats per partial, elements over all segments
    float clamp;
    const float* partial;
};

__global__ void __launch_bounds__(256) evg_qnet_grad_reduce_kernel(QnetGradReduceArgs a) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    int s = 0;
    while (s + 1 < a.nseg && e >= a.seg[s].rows * a.seg[s].cols) {
        e -= a.seg[s].rows * a.seg[s].cols;
        ++s;
    }
    const QnetGradSeg sg = a.seg[s];
    const int j = e / sg.cols, i = e - j * sg.cols;
    const float* __restrict__ p = a.partial + sg.src + j * sg.ld + i;
    float v = 0.0f;
    int b = 0;
    for (; b + 8 <= a.blocks; b += 8) {                 // (eight loads in flight; the additions keep their order)
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(long long)(b + u) * a.stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; b < a.blocks; ++b) v += p[(long long)b * a.stride];
    if (a.clamp > 0.0f) v = fminf(fmaxf(v, -a.clamp), a.clamp);
    sg.dst[e] = v;
}

// workgroups of a backward launch: a function of rows and the device's CU count alone
long long qnet_grad_blocks(long long rows, int num_cu) {
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (cap > EVG_QNET_GRAD_MAX_BLOCKS) cap = EVG_QNET_GRAD_MAX_BLOCKS;
    return blocks < cap ? blocks : cap;
}

static int launch_qnet_grad_reduce(QnetGradReduceArgs& r, hipStream_t s) {
    r.total = 0;
    for (int i = 0; i < r.nseg; ++i) r.total += r.seg[i].rows * r.seg[i].cols;
    hipLaunchKernelGGL(evg_qnet_grad_reduce_kernel, dim3((unsigned)((r.total + 255) / 256)), dim3(256), 0, s, r);
    return (int)hipGetLastError();
}

int launch_smart_qnet_backward(const evg_qnet& net, long long rows, const float* x, const float* gq, const evg_qnet_grads& out, float* workspace,
                               float clamp, int num_cu, void* stream) {
    QnetGradArgs a;
    a.W = QnetSet{net.w1[0], net.b1[0], net.w2[0], net.b2[0], net.w3[0], net.b3[0]};
    a.h1 = net.h1;
    a.h2 = net.h2;
    a.final_relu = net.final_relu;
    a.rows = rows;
    a.x = x;
    a.gq = gq;
    a.partial = workspace;
    const long long blocks = qnet_grad_blocks(rows, num_cu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_qnet_grad_kernel, dim3((unsigned)blocks), dim3(64 * QN_WAVES), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    QnetGradReduceArgs r;
    r.seg[0] = QnetGradSeg{out.w1, net.h1, QN_IN, 0, 64};
    r.seg[1] = QnetGradSeg{out.w2, net.h2, net.h1, 4096, 64};
    r.seg[2] = QnetGradSeg{out.w3, QN_OUT, net.h2, 8192, 64};
    r.seg[3] = QnetGradSeg{out.b1, 1, net.h1, 9216, 0};
    r.seg[4] = QnetGradSeg{out.b2, 1, net.h2, 9280, 0};
    r.seg[5] = QnetGradSeg{out.b3, 1, QN_OUT, 9344, 0};
    r.nseg = 6;
    r.blocks = (int)blocks;
    r.stride = QG_P;
    r.clamp = clamp;
    r.partial = workspace;
    return launch_qnet_grad_reduce(r, s);
}

int launch_minimized_qnet_backward(const evg_mini_qnet& net, long long rows, const float* x, const float* gq, const evg_mini_qnet_grads& out,
                                   float* workspace, float clamp, int num_cu, void* stream) {
    MiniQnetGradArgs a;
    a.W = MiniQnetSet{net.w1[0], net.b1[0], net.w2[0], net.b2[0]};
    a.h1 = net.h1;
    a.final_relu = net.final_relu;
    a.rows = rows;
    a.x = x;
    a.gq = gq;
    a.partial = workspace;
    const long long blocks = qnet_grad_blocks(rows, num_cu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_mini_qnet_grad_kernel, dim3((unsigned)blocks), dim3(64 * QN_WAVES), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    QnetGradReduceArgs r;
    r.seg[0] = QnetGradSeg{out.w1, net.h1, QN_IN, 0, 64};
    r.seg[1] = QnetGradSeg{out.w2, MQ_OUT, net.h1, 4 * MG_CHUNK, MQ_H};
    r.seg[2] = QnetGradSeg{out.b1, 1, net.h1, 5 * MG_CHUNK, 0};
    r.seg[3] = QnetGradSeg{out.b2, 1, MQ_OUT, 5 * MG_CHUNK + 128, 0};
    for (int i = 4; i < 6; ++i) r.seg[i] = QnetGradSeg{nullptr, 0, 0, 0, 0};
    r.nseg = 4;
    r.blocks = (int)blocks;
    r.stride = MG_P;
    r.clamp = clamp;
    r.partial = workspace;
    return launch_qnet_grad_reduce(r, s);
}
