// The learner step's glue (include/evg_learn.h, libevg_learn.so): the TD head -- target, Huber loss, dLoss/dQ -- and one Adam step over a network's
// tensors.  Included by evg_kernels.hip under EVG_LEARN.  Every arithmetic statement is one fp32 operation in the header's order (-ffp-contract=off).

struct LearnTdArgs {
    const float* q_pred;
    const long long* action;
    const float* q_next;
    const float* q_select;
    const float* reward;
    const uint8_t* not_done;
    const float* weights;
    float* gq;
    float* loss;
    float* priorities;
    float* estimated;
    float* partial;
    int batch, mode;
    float scale;
};

constexpr int LEARN_TD_THREADS = 256;                   // 16 slots of 16 lanes: a slot owns one sample at a time, lane s < 12 of it the swarm s
constexpr int LEARN_TD_SLOTS = LEARN_TD_THREADS / 16;

template <int OUT>
__global__ void __launch_bounds__(LEARN_TD_THREADS) evg_learn_td_head_kernel(LearnTdArgs a) {
    __shared__ float slot_sum[LEARN_TD_SLOTS];
    const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const int chunks = (a.batch + LEARN_TD_SLOTS - 1) / LEARN_TD_SLOTS;
    const float fB = (float)a.batch;
    float acc = 0.0f;                                   // this slot's sum of w * term, samples ascending (kept equal in its 16 lanes)
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {         // uniform over the workgroup; the shuffles below run with all 64 lanes active
        const int b = c * LEARN_TD_SLOTS + slot;
        const bool live = b < a.batch;
        float v = 0.0f;
        if (live && lane < EVG_TD_SWARMS) {
            const float* __restrict__ qn = a.q_next + ((long long)b * EVG_TD_SWARMS + lane) * OUT;
            if (a.mode == EVG_TD_DOUBLE_MEAN) {
                const float* __restrict__ qs = a.q_select + ((long long)b * EVG_TD_SWARMS + lane) * OUT;
                float best = qs[0];
                v = qn[0];
#pragma unroll
                for (int k = 1; k < OUT; ++k) {
                    const float s = qs[k], n = qn[k];
                    if (s > best) { best = s; v = n; }  // strictly greater: the first index of the maximum
                }
            } else {
                v = qn[0];
#pragma unroll
                for (int k = 1; k < OUT; ++k) v = fmaxf(v, qn[k]);
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
            if (valid) td = a.q_pred[(long long)b * OUT + act] - est;
            const float ad = fabsf(td);
            float term = ad < 1.0f ? (0.5f * td) * td : ad - 0.5f;
            float g = fminf(fmaxf(td, -1.0f), 1.0f);
            if (a.weights) {
                const float w = a.weights[b];
                term = w * term;
                g = w * g;
            }
            g = g / fB;
            if (lane < OUT) a.gq[(long long)b * OUT + lane] = (valid && lane == (int)act) ? g : 0.0f;
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
        a.partial[blockIdx.x] = s;
    }
}

// the G partials in a fixed order: lane l adds l, l + 64, ...; lane 0 then adds the 64 lanes' sums ascending and divides by B
__global__ void __launch_bounds__(64) evg_learn_td_loss_kernel(const float* __restrict__ partial, int blocks, int batch, float* __restrict__ loss) {
    __shared__ float lane_sum[64];
    float s = 0.0f;
    for (int i = threadIdx.x; i < blocks; i += 64) s = s + partial[i];
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = lane_sum[0];
        for (int k = 1; k < 64; ++k) t = t + lane_sum[k];
        loss[0] = t / (float)batch;
    }
}

int launch_td_head(const evg_td_head_args& d, void* stream) {
    LearnTdArgs a;
    a.q_pred = d.q_pred;
    a.action = reinterpret_cast<const long long*>(d.action);
    a.q_next = d.q_next;
    a.q_select = d.mode == EVG_TD_DOUBLE_MEAN ? d.q_select : nullptr;
    a.reward = d.reward;
    a.not_done = d.not_done;
    a.weights = d.weights;
    a.gq = d.gq;
    a.loss = d.loss;
    a.priorities = d.priorities;
    a.estimated = d.estimated;
    a.partial = static_cast<float*>(d.workspace);
    a.batch = d.batch;
    a.mode = d.mode;
    a.scale = d.scale;
    int blocks = (d.batch + LEARN_TD_SLOTS - 1) / LEARN_TD_SLOTS;
    if (blocks > EVG_TD_HEAD_MAX_BLOCKS) blocks = EVG_TD_HEAD_MAX_BLOCKS;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d.out == 5)
        hipLaunchKernelGGL(evg_learn_td_head_kernel<5>, dim3((unsigned)blocks), dim3(LEARN_TD_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(evg_learn_td_head_kernel<11>, dim3((unsigned)blocks), dim3(LEARN_TD_THREADS), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(evg_learn_td_loss_kernel, dim3(1), dim3(64), 0, s, a.partial, blocks, d.batch, d.loss);
    return (int)hipGetLastError();
}

// ---- Adam
struct LearnAdamCtl {
    long long step;
    double p1, p2;
    long long reserved;
};

struct LearnAdamArgs {
    evg_adam_tensor t[EVG_ADAM_MAX_TENSORS];
    LearnAdamCtl* ctl;
    int n, fresh;
    float lr, beta1, beta2, eps, clamp;
};

constexpr int LEARN_ADAM_THREADS = 1024;

// ONE workgroup (launch_adam_step): every thread reads ctl, all meet at the barrier after the element loop, thread 0 alone stores ctl after it
__global__ void __launch_bounds__(LEARN_ADAM_THREADS) evg_learn_adam_kernel(LearnAdamArgs a) {
    long long step = 0;
    double p1 = 1.0, p2 = 1.0;
    if (!a.fresh) {
        step = a.ctl->step;
        p1 = a.ctl->p1;
        p2 = a.ctl->p2;
    }
    p1 = p1 * (double)a.beta1;
    p2 = p2 * (double)a.beta2;
    const float step_size = (float)((double)a.lr / (1.0 - p1));
    const float bc2s = (float)sqrt(1.0 - p2);
    const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
    for (int i = 0; i < a.n; ++i) {
        const evg_adam_tensor t = a.t[i];
        for (long long e = threadIdx.x; e < t.count; e += LEARN_ADAM_THREADS) {
            float g = t.grad[e];
            if (a.clamp > 0.0f) g = fminf(fmaxf(g, -a.clamp), a.clamp);
            const float m0 = a.fresh ? 0.0f : t.m[e], v0 = a.fresh ? 0.0f : t.v[e];
            const float m1 = m0 + (g - m0) * omb1;
            const float v1 = a.beta2 * v0 + (omb2 * g) * g;
            const float den = sqrtf(v1) / bc2s + a.eps;
            t.m[e] = m1;
            t.v[e] = v1;
            t.param[e] = t.param[e] - step_size * (m1 / den);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.ctl->step = step + 1;
        a.ctl->p1 = p1;
        a.ctl->p2 = p2;
    }
}

int launch_adam_step(const evg_adam_args& d, void* stream) {
    LearnAdamArgs a;
    for (int i = 0; i < EVG_ADAM_MAX_TENSORS; ++i) a.t[i] = i < d.n ? d.t[i] : evg_adam_tensor{nullptr, nullptr, nullptr, nullptr, 0};
    a.ctl = static_cast<LearnAdamCtl*>(d.ctl);
    a.n = d.n;
    a.fresh = d.fresh_state != 0;
    a.lr = d.lr;
    a.beta1 = d.beta1;
    a.beta2 = d.beta2;
    a.eps = d.eps;
    a.clamp = d.clamp;
    hipLaunchKernelGGL(evg_learn_adam_kernel, dim3(1), dim3(LEARN_ADAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
