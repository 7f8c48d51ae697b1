// The agents/DQN family's learner step (include/evg_dqn_learn.h, libevg_dqnlearn.so): the top-7 TD head -- target, Huber / squared loss, dLoss/dQ -- and
// Adam over a large network launched over a grid.  Included by evg_kernels.hip under EVG_DQN_LEARN.  Every arithmetic statement is one fp32 operation in
// the header's order (-ffp-contract=off).

struct DqnTdArgs {
    const float* q_pred;
    const long long* action;
    const float* q_next;
    const float* reward;
    const uint8_t* not_done;
    const float* weights;
    float* gq;
    float* loss;
    float* priorities;
    float* estimated;
    float* partial;
    int batch, mode;
    float gamma;
};

constexpr int DQN_TD_THREADS = 256;                     // 16 slots of 16 lanes: a slot owns one sample at a time
constexpr int DQN_TD_SLOTS = DQN_TD_THREADS / 16;
constexpr int DQN_TD_OUT = 132;
constexpr int DQN_TD_REGS = 9;                          // lane l of a slot holds the elements l, l + 16, ..., l + 128 (>= 132: padding)

// the maximum over the 16 lanes of a DPP row, left in all of them: the lane pairs of a quad, the quad's halves, the row's half mirrored, the row mirrored
__device__ __forceinline__ float dqn_td_row_max(float v) {
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));      // quad_perm [1, 0, 3, 2]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));      // quad_perm [2, 3, 0, 1]
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));     // row_half_mirror
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));     // row_mirror
    return v;
}

__global__ void __launch_bounds__(DQN_TD_THREADS) evg_dqn_td_head_kernel(DqnTdArgs a) {
    __shared__ float slot_sum[DQN_TD_SLOTS];
    const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const int chunks = (a.batch + DQN_TD_SLOTS - 1) / DQN_TD_SLOTS;
    const float f7B = (float)(EVG_DQN_TD_ACTIONS * a.batch);
    const float NEG = -__builtin_inff();
    float acc = 0.0f;                                   // this slot's sum of rows, samples ascending (kept equal in its 16 lanes)
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {         // uniform over the workgroup: the cross-lane operations below run with all 64 lanes active
        const int b = c * DQN_TD_SLOTS + slot;
        const bool live = b < a.batch;
        float v[DQN_TD_REGS];
#pragma unroll
        for (int s = 0; s < DQN_TD_REGS; ++s) {
            const int e = lane + 16 * s;
            v[s] = (live && e < DQN_TD_OUT) ? a.q_next[(long long)b * DQN_TD_OUT + e] : NEG;
        }
        // seven rounds: each retires ONE instance of the row's maximum; lane j keeps round j's value
        float mine = 0.0f;
#pragma unroll
        for (int j = 0; j < EVG_DQN_TD_ACTIONS; ++j) {
            float lm = v[0];
#pragma unroll
            for (int s = 1; s < DQN_TD_REGS; ++s) lm = fmaxf(lm, v[s]);
            const float M = dqn_td_row_max(lm);
            const unsigned holders = (unsigned)(__ballot(lm == M) >> (threadIdx.x & 48)) & 0xFFFFu;     // this slot's lanes that hold the maximum
            bool retired = lane != __ffs(holders) - 1;                                                   // only the lowest of them retires ...
#pragma unroll
            for (int s = 0; s < DQN_TD_REGS; ++s) {                                                      // ... its first register equal to it
                const bool hit = !retired && v[s] == M;
                v[s] = hit ? NEG : v[s];
                retired = retired || hit;
            }
            if (lane == j) mine = M;
        }
        // pair j in lane j < 7
        float e = 0.0f, ad = 0.0f, g = 0.0f;
        int act = -1;
        if (live && lane < EVG_DQN_TD_ACTIONS) {
            float prod = mine * a.gamma;
            if (a.not_done && a.not_done[b] == 0) prod = 0.0f;
            const float est = prod + a.reward[b];
            const long long al = a.action[(long long)b * EVG_DQN_TD_ACTIONS + lane];
            const bool valid = al >= 0 && al < DQN_TD_OUT;
            float td = 0.0f;
            if (valid) {
                act = (int)al;
                td = a.q_pred[(long long)b * DQN_TD_OUT + act] - est;
            }
            ad = fabsf(td);
            if (a.mode == EVG_DQN_TD_SQUARED) {
                e = td * td;
                g = 2.0f * td;
                if (a.weights) {
                    const float w = a.weights[b];
                    e = e * w;
                    g = g * w;
                }
            } else {
                e = ad < 1.0f ? (0.5f * td) * td : ad - 0.5f;
                g = fminf(fmaxf(td, -1.0f), 1.0f);
                if (a.weights) {
                    const float w = a.weights[b];
                    e = w * e;
                    g = w * g;
                }
            }
            g = g / f7B;
            if (a.estimated) a.estimated[(long long)b * EVG_DQN_TD_ACTIONS + lane] = est;
        }
        // the row's sums, j ascending, and its gq row: lane l builds the elements l, l + 16, ... from the pairs' (action, g), j ascending
        float row = __shfl(e, 0, 16), sad = __shfl(ad, 0, 16);
        float gr[DQN_TD_REGS];
#pragma unroll
        for (int s = 0; s < DQN_TD_REGS; ++s) gr[s] = 0.0f;
#pragma unroll
        for (int j = 0; j < EVG_DQN_TD_ACTIONS; ++j) {
            if (j > 0) {
                row = row + __shfl(e, j, 16);
                sad = sad + __shfl(ad, j, 16);
            }
            const int aj = __shfl(act, j, 16);
            const float gj = __shfl(g, j, 16);
#pragma unroll
            for (int s = 0; s < DQN_TD_REGS; ++s)
                if (aj == lane + 16 * s) gr[s] = gr[s] + gj;
        }
        if (live) {
#pragma unroll
            for (int s = 0; s < DQN_TD_REGS; ++s) {
                const int el = lane + 16 * s;
                if (el < DQN_TD_OUT) a.gq[(long long)b * DQN_TD_OUT + el] = gr[s];
            }
            if (lane == 0 && a.priorities) a.priorities[b] = (a.mode == EVG_DQN_TD_SQUARED ? row : sad) / 7.0f + 1e-5f;
            acc = acc + row;
        }
    }
    if (lane == 0) slot_sum[slot] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = slot_sum[0];
#pragma unroll
        for (int k = 1; k < DQN_TD_SLOTS; ++k) s = s + slot_sum[k];
        a.partial[blockIdx.x] = s;
    }
}

// the G partials in a fixed order: lane l adds l, l + 64, ...; lane 0 then adds the 64 lanes' sums ascending and divides by 7B
__global__ void __launch_bounds__(64) evg_dqn_td_loss_kernel(const float* __restrict__ partial, int blocks, int batch, float* __restrict__ loss) {
    __shared__ float lane_sum[64];
    float s = 0.0f;
    for (int i = threadIdx.x; i < blocks; i += 64) s = s + partial[i];
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = lane_sum[0];
        for (int k = 1; k < 64; ++k) t = t + lane_sum[k];
        loss[0] = t / (float)(EVG_DQN_TD_ACTIONS * batch);
    }
}

int launch_dqn_td_head(const evg_dqn_td_head_args& d, void* stream) {
    DqnTdArgs a;
    a.q_pred = d.q_pred;
    a.action = reinterpret_cast<const long long*>(d.action);
    a.q_next = d.q_next;
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
    a.gamma = d.gamma;
    int blocks = (d.batch + DQN_TD_SLOTS - 1) / DQN_TD_SLOTS;
    if (blocks > EVG_DQN_TD_MAX_BLOCKS) blocks = EVG_DQN_TD_MAX_BLOCKS;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_dqn_td_head_kernel, dim3((unsigned)blocks), dim3(DQN_TD_THREADS), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(evg_dqn_td_loss_kernel, dim3(1), dim3(64), 0, s, a.partial, blocks, d.batch, d.loss);
    return (int)hipGetLastError();
}

// ---- Adam over a grid
struct AdamWideCtl {
    long long step;
    double p1, p2;
    long long reserved;
};

struct AdamWideArgs {
    evg_adam_tensor t[EVG_ADAM_MAX_TENSORS];
    long long first[EVG_ADAM_MAX_TENSORS + 1];          // tensor i owns the units first[i] .. first[i + 1] - 1 (four elements each, the last may be short)
    AdamWideCtl* ctl;
    int n, fresh;
    float lr, beta1, beta2, eps, clamp;
};

constexpr int ADAM_WIDE_THREADS = 256;

struct AdamWideTerms {
    float step_size, bc2s, omb1, omb2, beta2, eps, clamp;
    bool fresh;
};

// evg_adam_step's element, operation for operation
__device__ __forceinline__ void adam_wide_element(const AdamWideTerms& k, float g, float m0, float v0, float p0, float& m1, float& v1, float& p1) {
    if (k.clamp > 0.0f) g = fminf(fmaxf(g, -k.clamp), k.clamp);
    if (k.fresh) {
        m0 = 0.0f;
        v0 = 0.0f;
    }
    m1 = m0 + (g - m0) * k.omb1;
    v1 = k.beta2 * v0 + (k.omb2 * g) * g;
    const float den = sqrtf(v1) / k.bc2s + k.eps;
    p1 = p0 - k.step_size * (m1 / den);
}

// reads ctl, never writes it: evg_adam_wide_ctl_kernel advances it after this launch has finished
__global__ void __launch_bounds__(ADAM_WIDE_THREADS) evg_adam_wide_kernel(AdamWideArgs a) {
    double p1 = 1.0, p2 = 1.0;
    if (!a.fresh) {
        p1 = a.ctl->p1;
        p2 = a.ctl->p2;
    }
    p1 = p1 * (double)a.beta1;
    p2 = p2 * (double)a.beta2;
    AdamWideTerms k;
    k.step_size = (float)((double)a.lr / (1.0 - p1));
    k.bc2s = (float)sqrt(1.0 - p2);
    k.omb1 = 1.0f - a.beta1;
    k.omb2 = 1.0f - a.beta2;
    k.beta2 = a.beta2;
    k.eps = a.eps;
    k.clamp = a.clamp;
    k.fresh = a.fresh != 0;
    // a thread's flat unit indices u, u + stride, ... ascend, so one running index walks the tensors in order: the tensor loop is uniform and its
    // descriptor a scalar load
    const long long stride = (long long)gridDim.x * ADAM_WIDE_THREADS;
    long long u = (long long)blockIdx.x * ADAM_WIDE_THREADS + threadIdx.x;
    for (int i = 0; i < a.n; ++i) {
        const evg_adam_tensor t = a.t[i];
        const long long base = a.first[i], end = a.first[i + 1];
        for (; u < end; u += stride) {
            const long long e0 = (u - base) * 4;
            if (e0 + 4 <= t.count) {
                const float4 g = *reinterpret_cast<const float4*>(t.grad + e0);
                float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = m;
                if (!k.fresh) {
                    m = *reinterpret_cast<const float4*>(t.m + e0);
                    v = *reinterpret_cast<const float4*>(t.v + e0);
                }
                float4 p = *reinterpret_cast<const float4*>(t.param + e0);
                adam_wide_element(k, g.x, m.x, v.x, p.x, m.x, v.x, p.x);
                adam_wide_element(k, g.y, m.y, v.y, p.y, m.y, v.y, p.y);
                adam_wide_element(k, g.z, m.z, v.z, p.z, m.z, v.z, p.z);
                adam_wide_element(k, g.w, m.w, v.w, p.w, m.w, v.w, p.w);
                *reinterpret_cast<float4*>(t.m + e0) = m;
                *reinterpret_cast<float4*>(t.v + e0) = v;
                *reinterpret_cast<float4*>(t.param + e0) = p;
            } else {
                for (long long e = e0; e < t.count; ++e) {          // the tensor's short last unit: one to three elements
                    float m1, v1, q1;
                    adam_wide_element(k, t.grad[e], k.fresh ? 0.0f : t.m[e], k.fresh ? 0.0f : t.v[e], t.param[e], m1, v1, q1);
                    t.m[e] = m1;
                    t.v[e] = v1;
                    t.param[e] = q1;
                }
            }
        }
    }
}

// one thread, launched behind the element kernel on the same stream: ctl advances exactly once per call, after its last reader
__global__ void __launch_bounds__(64) evg_adam_wide_ctl_kernel(AdamWideCtl* ctl, int fresh, float beta1, float beta2) {
    if (threadIdx.x != 0) return;
    long long step = 0;
    double p1 = 1.0, p2 = 1.0;
    if (!fresh) {
        step = ctl->step;
        p1 = ctl->p1;
        p2 = ctl->p2;
    }
    ctl->step = step + 1;
    ctl->p1 = p1 * (double)beta1;
    ctl->p2 = p2 * (double)beta2;
}

int launch_adam_step_wide(const evg_adam_args& d, void* stream) {
    AdamWideArgs a;
    long long units = 0;
    for (int i = 0; i < EVG_ADAM_MAX_TENSORS; ++i) {
        a.t[i] = i < d.n ? d.t[i] : evg_adam_tensor{nullptr, nullptr, nullptr, nullptr, 0};
        a.first[i] = units;
        if (i < d.n) units += (d.t[i].count + 3) / 4;
    }
    a.first[EVG_ADAM_MAX_TENSORS] = units;
    for (int i = d.n; i < EVG_ADAM_MAX_TENSORS; ++i) a.first[i] = units;
    a.ctl = static_cast<AdamWideCtl*>(d.ctl);
    a.n = d.n;
    a.fresh = d.fresh_state != 0;
    a.lr = d.lr;
    a.beta1 = d.beta1;
    a.beta2 = d.beta2;
    a.eps = d.eps;
    a.clamp = d.clamp;
    long long blocks = (units + ADAM_WIDE_THREADS - 1) / ADAM_WIDE_THREADS;
    if (blocks > EVG_ADAM_WIDE_MAX_BLOCKS) blocks = EVG_ADAM_WIDE_MAX_BLOCKS;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evg_adam_wide_kernel, dim3((unsigned)blocks), dim3(ADAM_WIDE_THREADS), 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(evg_adam_wide_ctl_kernel, dim3(1), dim3(64), 0, s, a.ctl, a.fresh, d.beta1, d.beta2);
    return (int)hipGetLastError();
}
