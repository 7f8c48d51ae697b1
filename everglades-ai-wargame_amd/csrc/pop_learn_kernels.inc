// pop_learn_kernels.inc -- self-royale: the grouped forms of the learner step's kernels (include/evg_pop_learn.h, libevg_poplearn.so): one sampled batch
// trains every member of one team, each row routed to the member that played it.  Included by evg_kernels.hip (namespace evg) under EVG_POP_LEARN (with
// EVG_GRAD and EVG_LEARN), after population_kernels.inc, qnet_grad_kernels.inc and learn_kernels.inc, whose constants, argument sets and helpers it uses.
//
//   evg_poplearn_expand_ids_kernel          a transition's id for each of its next-state rows
//   evg_poplearn_take_rows_kernel           one member's rows out of a whole-batch forward (the bf16 targets: one plain forward per member)
//   evg_poplearn_td_head_kernel<OUT>        evg_learn_td_head_kernel over a member's list as a batch of c_m (blockIdx.y = member; the last row of the
//                                           grid takes bin 16, the rows of no member: zeros)
//   evg_poplearn_td_loss_kernel             evg_learn_td_loss_kernel per member (blockIdx.x = member)
//   evg_poplearn_qnet_grad_kernel           evg_qnet_grad_kernel's body (qnet_grad_body.inc, QG_GROUPED 1) with the grouped forwards' prologue
//   evg_poplearn_mini_qnet_grad_kernel      the same for evg_mini_qnet_grad_kernel (minimized_qnet_grad_body.inc)
//   evg_poplearn_grad_reduce_kernel         per member, its workgroups' partials in ascending order -> clamp -> the member's gradient tensors
//   evg_poplearn_adam_kernel                evg_learn_adam_kernel, workgroup m over member m's tensors and control block; c_m = 0 leaves at once
//
// Who owns a row is read from the bucket pass of the policy population's expanded forward (population_kernels.inc: index / first / count, seat slot 0).
// No kernel here has a floating-point atomic: every sum's order is a function of the ids and the grid.

struct PopLists {
    const int32_t* index;
    const int32_t* first;
    const int32_t* count;
    int32_t num, rows;
};

// bin `bin`'s extent, clamped into the list as the grouped forwards clamp it
__device__ __forceinline__ long long pl_extent(const PopLists& L, int bin, long long& first) {
    const long long rows = L.rows;
    long long cnt = L.count[bin];
    cnt = cnt < rows ? cnt : rows;
    if (cnt <= 0) {
        first = 0;
        return 0;
    }
    long long f = L.first[bin];
    first = f < 0 ? 0 : (f < rows - cnt ? f : rows - cnt);
    return cnt;
}

// the workgroups of a grid row of gx that member `bin`'s cnt rows use: the grouped forward's share
__device__ __forceinline__ long long pl_live(const PopLists& L, long long cnt, long long gx) {
    if (cnt <= 0) return 0;
    const long long need = (cnt + 16 * QN_WAVES - 1) / (16 * QN_WAVES);
    const long long live = (gx * cnt + L.rows - 1) / L.rows;
    return live < need ? live : need;
}

// the partials of the members before `member`: where this member's begin in the packed workspace
__device__ __forceinline__ long long pl_base(const PopLists& L, int member, long long gx) {
    long long base = 0;
    for (int j = 0; j < member; ++j) {
        long long f;
        base += pl_live(L, pl_extent(L, j, f), gx);
    }
    return base;
}

__global__ void __launch_bounds__(256) evg_poplearn_expand_ids_kernel(const uint8_t* __restrict__ member, int batch, int repeat, uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)batch * repeat) out[i] = member[i / repeat];
}

// One thread per element of [rows][width]: a row of `member` is taken from src, a row of nobody (id >= num) is zeroed, every other row is left as it is.
__global__ void __launch_bounds__(256) evg_poplearn_take_rows_kernel(const float* __restrict__ src, const uint8_t* __restrict__ ids, int member, int num,
                                                                     long long rows, int width, float* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * width) return;
    const int id = ids[i / width];
    if (id == member)
        dst[i] = src[i];
    else if (id >= num)
        dst[i] = 0.0f;
}

// ---- the TD head
struct PopTdArgs {
    LearnTdArgs t;                                      // loss [K]; partial [K][EVG_TD_HEAD_MAX_BLOCKS]
    PopLists L;
};

template <int OUT>
__global__ void __launch_bounds__(LEARN_TD_THREADS) evg_poplearn_td_head_kernel(PopTdArgs p) {
    __shared__ float slot_sum[LEARN_TD_SLOTS];
    const LearnTdArgs& a = p.t;
    const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const bool nobody = (int)blockIdx.y >= p.L.num;
    const int bin = nobody ? EVG_POP_MAX_MEMBERS : (int)blockIdx.y;
    long long first;
    const long long cnt = pl_extent(p.L, bin, first);
    if (cnt <= 0) return;
    const int batch = (int)cnt;                         // the member's rows as a batch of their own
    const int chunks = (batch + LEARN_TD_SLOTS - 1) / LEARN_TD_SLOTS;
    const int G = chunks < EVG_TD_HEAD_MAX_BLOCKS ? chunks : EVG_TD_HEAD_MAX_BLOCKS;
    if ((int)blockIdx.x >= G) return;                   // (uniform: before any shuffle or barrier)
    const int* const list = p.L.index + first;
    if (nobody) {                                       // rows of no member: a zero gq row, priority 0, in no sum
        for (int c = blockIdx.x; c < chunks; c += G) {
            const int k = c * LEARN_TD_SLOTS + slot;
            if (k < batch) {
                const long long b = mq_list_row(list, k, p.L.rows);
                if (lane < OUT) a.gq[b * OUT + lane] = 0.0f;
                if (lane == 0) {
                    if (a.priorities) a.priorities[b] = 0.0f;
                    if (a.estimated) a.estimated[b] = 0.0f;
                }
            }
        }
        return;
    }
    const float fB = (float)batch;
    float acc = 0.0f;                                   // this slot's sum of w * term, list positions ascending (kept equal in its 16 lanes)
    for (int c = blockIdx.x; c < chunks; c += G) {      // uniform over the workgroup; the shuffles below run with all 64 lanes active
        const int k = c * LEARN_TD_SLOTS + slot;
        const bool live = k < batch;
        const long long b = live ? mq_list_row(list, k, p.L.rows) : 0;
        float v = 0.0f;
        if (live && lane < EVG_TD_SWARMS) {
            const float* __restrict__ qn = a.q_next + (b * EVG_TD_SWARMS + lane) * OUT;
            if (a.mode == EVG_TD_DOUBLE_MEAN) {
                const float* __restrict__ qs = a.q_select + (b * EVG_TD_SWARMS + lane) * OUT;
                float best = qs[0];
                v = qn[0];
#pragma unroll
                for (int o = 1; o < OUT; ++o) {
                    const float s = qs[o], n = qn[o];
                    if (s > best) { best = s; v = n; }  // strictly greater: the first index of the maximum
                }
            } else {
                v = qn[0];
#pragma unroll
                for (int o = 1; o < OUT; ++o) v = fmaxf(v, qn[o]);
            }
        }
        float future = __shfl(v, 0, 16);
        if (a.mode == EVG_TD_MAX_MAX) {
#pragma unroll
            for (int s = 1; s < EVG_TD_SWARMS; ++s) future = fmaxf(future, __shfl(v, s, 16));
        } else {
#pragma unroll
            for (int s = 1; s < EVG_TD_SWARMS; ++s) future = future + __shfl(v, s, 16);
            future = future / 12.0f;
        }
        if (live) {
            if (a.not_done[b] == 0) future = 0.0f;
            const float est = fmaf(future, a.scale, a.reward[b]);
            const long long act = a.action[b];
            const bool valid = act >= 0 && act < OUT;
            float td = 0.0f;
            if (valid) td = a.q_pred[b * OUT + act] - est;
            const float ad = fabsf(td);
            float term = ad < 1.0f ? (0.5f * td) * td : ad - 0.5f;
            float g = fminf(fmaxf(td, -1.0f), 1.0f);
            if (a.weights) {
                const float w = a.weights[b];
                term = w * term;
                g = w * g;
            }
            g = g / fB;
            if (lane < OUT) a.gq[b * OUT + lane] = (valid && lane == (int)act) ? g : 0.0f;
            if (lane == 0) {
                if (a.priorities) a.priorities[b] = ad + 1e-5f;
                if (a.estimated) a.estimated[b] = est;
            }
            acc = acc + term;
        }
    }
    if (lane == 0) slot_sum[slot] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = slot_sum[0];
#pragma unroll
        for (int k = 1; k < LEARN_TD_SLOTS; ++k) s = s + slot_sum[k];
        a.partial[(long long)bin * EVG_TD_HEAD_MAX_BLOCKS + blockIdx.x] = s;
    }
}

// member m's G_m partials in evg_learn_td_loss_kernel's order, divided by c_m; 0 for a member without rows
__global__ void __launch_bounds__(64) evg_poplearn_td_loss_kernel(const float* __restrict__ partial, PopLists L, float* __restrict__ loss) {
    __shared__ float lane_sum[64];
    const int m = blockIdx.x;
    long long first;
    const long long cnt = pl_extent(L, m, first);
    const int chunks = (int)((cnt + LEARN_TD_SLOTS - 1) / LEARN_TD_SLOTS);
    const int blocks = chunks < EVG_TD_HEAD_MAX_BLOCKS ? chunks : EVG_TD_HEAD_MAX_BLOCKS;
    const float* __restrict__ pm = partial + (long long)m * EVG_TD_HEAD_MAX_BLOCKS;
    float s = 0.0f;
    for (int i = threadIdx.x; i < blocks; i += 64) s = s + pm[i];
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = lane_sum[0];
        for (int k = 1; k < 64; ++k) t = t + lane_sum[k];
        loss[m] = cnt > 0 ? t / (float)(int)cnt : 0.0f;
    }
}

int launch_td_head_grouped(const evg_td_head_grouped_args& d, void* stream) {
    PopTdArgs p;
    LearnTdArgs& a = p.t;
    a.q_pred = d.td.q_pred;
    a.action = reinterpret_cast<const long long*>(d.td.action);
    a.q_next = d.td.q_next;
    a.q_select = d.td.mode == EVG_TD_DOUBLE_MEAN ? d.td.q_select : nullptr;
    a.reward = d.td.reward;
    a.not_done = d.td.not_done;
    a.weights = d.td.weights;
    a.gq = d.td.gq;
    a.loss = d.td.loss;
    a.priorities = d.td.priorities;
    a.estimated = d.td.estimated;
    a.partial = static_cast<float*>(d.td.workspace);
    a.batch = d.td.batch;
    a.mode = d.td.mode;
    a.scale = d.td.scale;
    p.L = PopLists{d.lists.index, d.lists.first, d.lists.count, d.lists.num_members, d.lists.batch};
    int blocks = (d.td.batch + LEARN_TD_SLOTS - 1) / LEARN_TD_SLOTS;
    if (blocks > EVG_TD_HEAD_MAX_BLOCKS) blocks = EVG_TD_HEAD_MAX_BLOCKS;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)(p.L.num + 1));
    if (d.td.out == 5)
        hipLaunchKernelGGL(evg_poplearn_td_head_kernel<5>, grid, dim3(LEARN_TD_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(evg_poplearn_td_head_kernel<11>, grid, dim3(LEARN_TD_THREADS), 0, s, p);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(evg_poplearn_td_loss_kernel, dim3((unsigned)p.L.num), dim3(64), 0, s, a.partial, p.L, d.td.loss);
    return (int)hipGetLastError();
}

int launch_pop_expand_ids(const uint8_t* member, int batch, int repeat, uint8_t* out, void* stream) {
    const long long n = (long long)batch * repeat;
    hipLaunchKernelGGL(evg_poplearn_expand_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), member, batch,
                       repeat, out);
    return (int)hipGetLastError();
}

int launch_pop_take_rows(const float* src, const uint8_t* ids, int member, int num, long long rows, int width, float* dst, void* stream) {
    const long long n = rows * width;
    hipLaunchKernelGGL(evg_poplearn_take_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, ids,
                       member, num, rows, width, dst);
    return (int)hipGetLastError();
}

// ---- the backward
struct PopGradArgs {
    QnetGradArgs q;                                     // (its W is not read: the sets are below)
    QnetSet set[EVG_POP_MAX_MEMBERS];
    PopLists L;
};

__global__ void __launch_bounds__(64 * QN_WAVES) evg_poplearn_qnet_grad_kernel(PopGradArgs pa) {
    __shared__ __attribute__((aligned(16))) float lds[QG_LDS];
    // the grouped forwards' prologue: the member's count first; a workgroup outside the member's share leaves here, uniformly, before any staging
    const int member = blockIdx.y;
    long long first;
    const long long cnt = pl_extent(pa.L, member, first);
    const long long live = pl_live(pa.L, cnt, gridDim.x);
    if ((long long)blockIdx.x >= live) return;
    const long long part_slot = pl_base(pa.L, member, gridDim.x) + blockIdx.x;
    if (part_slot >= (long long)gridDim.x + pa.L.num) return;     // (counts that are no bucket pass's: nothing outside the workspace)
    const QnetGradArgs& a = pa.q;
    const QnetSet W = pa.set[member];
    const int* const list = pa.L.index + first;
    const long long list_rows = cnt, list_stride = live * QN_WAVES;
#define QG_GROUPED 1
#include "qnet_grad_body.inc"
#undef QG_GROUPED
}

struct PopMiniGradArgs {
    MiniQnetGradArgs q;
    MiniQnetSet set[EVG_POP_MAX_MEMBERS];
    PopLists L;
};

__global__ void __launch_bounds__(64 * QN_WAVES) evg_poplearn_mini_qnet_grad_kernel(PopMiniGradArgs pa) {
    __shared__ __attribute__((aligned(16))) float lds[MQ_H * MQ_W1S + QN_WAVES * 16 * MQ_HS];
    const int member = blockIdx.y;
    long long first;
    const long long cnt = pl_extent(pa.L, member, first);
    const long long live = pl_live(pa.L, cnt, gridDim.x);
    if ((long long)blockIdx.x >= live) return;
    const long long part_slot = pl_base(pa.L, member, gridDim.x) + blockIdx.x;
    if (part_slot >= (long long)gridDim.x + pa.L.num) return;
    const MiniQnetGradArgs& a = pa.q;
    const MiniQnetSet W = pa.set[member];
    const int* const list = pa.L.index + first;
    const long long list_rows = cnt, list_stride = live * QN_WAVES;
#define QG_GROUPED 1
#include "minimized_qnet_grad_body.inc"
#undef QG_GROUPED
}

// One thread per element of one member's gradient tensors (blockIdx.y = member): the sum of that element over the member's partials in ascending
// workgroup order, the optional clamp, one store.  A member without rows has no partial: zeros.
struct PopGradSeg {
    int rows, cols, src, ld;                            // element [j][i] is partial[src + j * ld + i]
};

struct PopGradReduceArgs {
    float* dst[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    PopGradSeg seg[EVG_POP_LEARN_MAX_TENSORS];
    int nseg, stride, total, gx;                        // floats per partial, elements over all segments, the backward's gridDim.x
    float clamp;
    const float* partial;
    PopLists L;
};

__global__ void __launch_bounds__(256) evg_poplearn_grad_reduce_kernel(PopGradReduceArgs a) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    const int member = blockIdx.y;
    int s = 0;
    while (s + 1 < a.nseg && e >= a.seg[s].rows * a.seg[s].cols) {
        e -= a.seg[s].rows * a.seg[s].cols;
        ++s;
    }
    const PopGradSeg sg = a.seg[s];
    long long first;
    const long long cnt = pl_extent(a.L, member, first);
    const long long base = pl_base(a.L, member, a.gx), room = (long long)a.gx + a.L.num - base;
    long long mine = pl_live(a.L, cnt, a.gx);
    mine = mine < room ? mine : room;                   // (what the backward's workgroups wrote: those inside the workspace)
    const int blocks = mine > 0 ? (int)mine : 0;
    const int j = e / sg.cols, i = e - j * sg.cols;
    const float* __restrict__ p = a.partial + base * a.stride + sg.src + j * sg.ld + i;
    float v = 0.0f;
    int b = 0;
    for (; b + 8 <= blocks; b += 8) {                   // (eight loads in flight; the additions keep their order)
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(long long)(b + u) * a.stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; b < blocks; ++b) v += p[(long long)b * a.stride];
    if (a.clamp > 0.0f) v = fminf(fmaxf(v, -a.clamp), a.clamp);
    a.dst[s][member][e] = v;
}

static int launch_pop_grad_reduce(PopGradReduceArgs& r, const evg_pop_backward_args& d, int nseg, hipStream_t s) {
    r.nseg = nseg;
    r.total = 0;
    for (int i = 0; i < EVG_POP_LEARN_MAX_TENSORS; ++i)
        for (int m = 0; m < EVG_POP_MAX_MEMBERS; ++m) r.dst[i][m] = (i < nseg && m < d.lists.num_members) ? d.grad[i][m] : nullptr;
    for (int i = 0; i < nseg; ++i) r.total += r.seg[i].rows * r.seg[i].cols;
    for (int i = nseg; i < EVG_POP_LEARN_MAX_TENSORS; ++i) r.seg[i] = PopGradSeg{0, 0, 0, 0};
    r.clamp = d.clamp;
    r.partial = static_cast<const float*>(d.workspace);
    r.L = PopLists{d.lists.index, d.lists.first, d.lists.count, d.lists.num_members, d.lists.batch};
    hipLaunchKernelGGL(evg_poplearn_grad_reduce_kernel, dim3((unsigned)((r.total + 255) / 256), (unsigned)d.lists.num_members), dim3(256), 0, s, r);
    return (int)hipGetLastError();
}

int launch_smart_population_backward(const evg_pop_backward_args& d, int num_cu, void* stream) {
    PopGradArgs p;
    const int K = d.lists.num_members;
    p.q.W = QnetSet{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    p.q.h1 = d.h1;
    p.q.h2 = d.h2;
    p.q.final_relu = d.final_relu;
    p.q.rows = d.lists.batch;
    p.q.x = d.x;
    p.q.gq = d.gq;
    p.q.partial = static_cast<float*>(d.workspace);
    for (int m = 0; m < EVG_POP_MAX_MEMBERS; ++m)
        p.set[m] = m < K ? QnetSet{d.param[0][m], d.param[1][m], d.param[2][m], d.param[3][m], d.param[4][m], d.param[5][m]}
                         : QnetSet{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    p.L = PopLists{d.lists.index, d.lists.first, d.lists.count, K, d.lists.batch};
    const long long gx = qnet_grad_blocks(d.lists.batch, num_cu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_poplearn_qnet_grad_kernel, dim3((unsigned)gx, (unsigned)K), dim3(64 * QN_WAVES), 0, s, p);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    PopGradReduceArgs r;
    r.seg[0] = PopGradSeg{d.h1, QN_IN, 0, 64};          // w1, b1, w2, b2, w3, b3: the order of evg_pop_backward_args.grad
    r.seg[1] = PopGradSeg{1, d.h1, 9216, 0};
    r.seg[2] = PopGradSeg{d.h2, d.h1, 4096, 64};
    r.seg[3] = PopGradSeg{1, d.h2, 9280, 0};
    r.seg[4] = PopGradSeg{QN_OUT, d.h2, 8192, 64};
    r.seg[5] = PopGradSeg{1, QN_OUT, 9344, 0};
    r.stride = QG_P;
    r.gx = (int)gx;
    return launch_pop_grad_reduce(r, d, 6, s);
}

int launch_population_backward(const evg_pop_backward_args& d, int num_cu, void* stream) {
    PopMiniGradArgs p;
    const int K = d.lists.num_members;
    p.q.W = MiniQnetSet{nullptr, nullptr, nullptr, nullptr};
    p.q.h1 = d.h1;
    p.q.final_relu = d.final_relu;
    p.q.rows = d.lists.batch;
    p.q.x = d.x;
    p.q.gq = d.gq;
    p.q.partial = static_cast<float*>(d.workspace);
    for (int m = 0; m < EVG_POP_MAX_MEMBERS; ++m)
        p.set[m] = m < K ? MiniQnetSet{d.param[0][m], d.param[1][m], d.param[2][m], d.param[3][m]} : MiniQnetSet{nullptr, nullptr, nullptr, nullptr};
    p.L = PopLists{d.lists.index, d.lists.first, d.lists.count, K, d.lists.batch};
    const long long gx = qnet_grad_blocks(d.lists.batch, num_cu);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_poplearn_mini_qnet_grad_kernel, dim3((unsigned)gx, (unsigned)K), dim3(64 * QN_WAVES), 0, s, p);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    PopGradReduceArgs r;
    r.seg[0] = PopGradSeg{d.h1, QN_IN, 0, 64};          // w1, b1, w2, b2
    r.seg[1] = PopGradSeg{1, d.h1, 5 * MG_CHUNK, 0};
    r.seg[2] = PopGradSeg{MQ_OUT, d.h1, 4 * MG_CHUNK, MQ_H};
    r.seg[3] = PopGradSeg{1, MQ_OUT, 5 * MG_CHUNK + 128, 0};
    r.stride = MG_P;
    r.gx = (int)gx;
    return launch_pop_grad_reduce(r, d, 4, s);
}

// ---- Adam
struct PopAdamArgs {
    float* param[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    const float* grad[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    float* m[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    float* v[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    long long elements[EVG_POP_LEARN_MAX_TENSORS];
    LearnAdamCtl* ctl;
    const int32_t* count;
    int n, fresh;
    float lr, beta1, beta2, eps, clamp;
};

// workgroup m is evg_learn_adam_kernel over member m: every thread reads the member's ctl, all meet at the barrier after the element loop, thread 0
// alone stores it after that.  No other workgroup touches that block.  A member without rows: nothing is read or written.
__global__ void __launch_bounds__(LEARN_ADAM_THREADS) evg_poplearn_adam_kernel(PopAdamArgs a) {
    const int mb = blockIdx.x;
    if (a.count[mb] <= 0) return;                       // (uniform over the workgroup)
    LearnAdamCtl* const ctl = a.ctl + mb;
    long long step = 0;
    double p1 = 1.0, p2 = 1.0;
    if (!a.fresh) {
        step = ctl->step;
        p1 = ctl->p1;
        p2 = ctl->p2;
    }
    p1 = p1 * (double)a.beta1;
    p2 = p2 * (double)a.beta2;
    const float step_size = (float)((double)a.lr / (1.0 - p1));
    const float bc2s = (float)sqrt(1.0 - p2);
    const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
    for (int i = 0; i < a.n; ++i) {
        float* const tp = a.param[i][mb];
        const float* const tg = a.grad[i][mb];
        float* const tm = a.m[i][mb];
        float* const tv = a.v[i][mb];
        const long long count = a.elements[i];
        for (long long e = threadIdx.x; e < count; e += LEARN_ADAM_THREADS) {
            float g = tg[e];
            if (a.clamp > 0.0f) g = fminf(fmaxf(g, -a.clamp), a.clamp);
            const float m0 = a.fresh ? 0.0f : tm[e], v0 = a.fresh ? 0.0f : tv[e];
            const float m1 = m0 + (g - m0) * omb1;
            const float v1 = a.beta2 * v0 + (omb2 * g) * g;
            const float den = sqrtf(v1) / bc2s + a.eps;
            tm[e] = m1;
            tv[e] = v1;
            tp[e] = tp[e] - step_size * (m1 / den);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ctl->step = step + 1;
        ctl->p1 = p1;
        ctl->p2 = p2;
    }
}

int launch_adam_step_grouped(const evg_adam_grouped_args& d, void* stream) {
    PopAdamArgs a;
    for (int i = 0; i < EVG_POP_LEARN_MAX_TENSORS; ++i) {
        a.elements[i] = i < d.n ? d.elements[i] : 0;
        for (int m = 0; m < EVG_POP_MAX_MEMBERS; ++m) {
            const bool on = i < d.n && m < d.num_members;
            a.param[i][m] = on ? d.param[i][m] : nullptr;
            a.grad[i][m] = on ? d.grad[i][m] : nullptr;
            a.m[i][m] = on ? d.m[i][m] : nullptr;
            a.v[i][m] = on ? d.v[i][m] : nullptr;
        }
    }
    a.ctl = static_cast<LearnAdamCtl*>(d.ctl);
    a.count = d.count;
    a.n = d.n;
    a.fresh = d.fresh_state != 0;
    a.lr = d.lr;
    a.beta1 = d.beta1;
    a.beta2 = d.beta2;
    a.eps = d.eps;
    a.clamp = d.clamp;
    hipLaunchKernelGGL(evg_poplearn_adam_kernel, dim3((unsigned)d.num_members), dim3(LEARN_ADAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
