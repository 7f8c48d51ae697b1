// population_kernels.inc -- self-royale (include/evg.h, evg_population): a per-env Minimized Q network drawn from a population each episode
// (agents/Minimized/training_scripts/dqn_self_royale.py: random.choice(team) per seat and episode).  Included by evg_kernels.hip inside namespace evg, after
// minimized_qnet.inc, whose body (minimized_qnet_body.inc) the grouped forward shares.  No step kernel knows about any of this:
//
//   evg_population_clear_kernel     one thread per env: both seats' members drawn for the env's current episode
//   evg_population_assign_kernel    one thread per env of the mask: history, per-member tally (the league's pattern: ballot + popcount, lane 0 adds),
//                                   then the draw for the episode the handle names
//   evg_population_hist_kernel      bucket pass 1: per-block (256 rows) counts of every member id, by wave ballot + popcount
//   evg_population_scan_kernel      bucket pass 2: one workgroup per seat slot scans the block counts bin after bin (evg_replay_top_kernel's pattern):
//                                   hist becomes each block's first position in the list, first / count the bins' extents
//   evg_population_scatter_kernel   bucket pass 3: row -> index[its block's position + counts of the waves before + rank inside the wave (mbcnt)].  No
//                                   global atomics anywhere, so the list is the stable order: rows ascending inside a member.  Rows whose id is >= K (bin
//                                   16) get zeros in q_out and set EVG_POP_S_BAD_MEMBER; they are in no member's list.  The layout follows the CALL
//                                   (include/evg.h): seat slot s's list begins at index + s * rows and hist is [S][17][nb], with that call's rows and
//                                   nb = ceil(rows / 256); the descriptor's scratch_rows bounds both and is no stride
//   evg_mini_qnet_pop_kernel<EXPANDED>   evg_mini_qnet_kernel with a workgroup belonging to one (seat slot, member): it stages that member's weights once
//                                   and runs the shared body over the member's list, reading rows through it and writing Q to their original positions
//   evg_qnet_pop_kernel<EXPANDED>   the same for the Smart_State network (evg_smart_population): evg_qnet_kernel's body (qnet_body.inc) over a member's
//                                   list.  Its assignment and bucket pass are the kernels above, unchanged (row_floats 5 / 60)
//
// The draw (RNG domain 6 = RNG_POPULATION, DESIGN.md section 4; tests/population_model.py is the host statement): member = mulhi32(w, K) with w = word .x
// of the block (domain 6, block 0, turn 0, node 0, player = seat, group 0, episode, env id) -- the form the combat draw uses; K = 1 draws nothing.

constexpr int POP_BINS = EVG_POP_MAX_MEMBERS + 1;      // the members and the bin of ids >= K
constexpr int POP_BLOCK = 256;                         // rows per workgroup of the bucket pass

struct PopArgs {                 // evg_population as the assignment kernels take it
    uint8_t* member;
    unsigned long long* counts;
    unsigned long long* ctl;
    int32_t num0, num1;
};

__device__ __forceinline__ int pop_draw(const DevState& S, int e, int player, int K) {
    if (K <= 1) return 0;
    const uint4 b = rng_block(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, S.episode[e], RNG_POPULATION, 0u, 0, 0, player, 0);
    return (int)__umulhi(b.x, (uint32_t)K);
}

// counts and ctl are zeroed by a memset ahead of this kernel (launch_population_clear)
__global__ void __launch_bounds__(256) evg_population_clear_kernel(DevState S, PopArgs g) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S.N) return;
    g.member[2 * e] = (uint8_t)pop_draw(S, e, 0, g.num0);
    g.member[2 * e + 1] = (uint8_t)pop_draw(S, e, 1, g.num1);
}

__global__ void __launch_bounds__(256) evg_population_assign_kernel(DevState S, PopArgs g, const uint8_t* mask, const int8_t* winner, uint8_t* history) {
    const int e = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool act = e < S.N && (!mask || mask[e]);           // (no early return: the tally's ballots are over whole wavefronts)
    int m[2] = {0, 0};
    if (act) {
        m[0] = g.member[2 * e];
        m[1] = g.member[2 * e + 1];
        if (history) {
            history[2 * e] = (uint8_t)m[0];
            history[2 * e + 1] = (uint8_t)m[1];
        }
    }
    if (winner) {
        const int w = act ? (int)winner[e] : (int)EVG_WINNER_NONE;
        const bool played = w == EVG_WINNER_P0 || w == EVG_WINNER_P1 || w == EVG_WINNER_TIE;
        bool bad = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool ok = played && m[p] < (p ? g.num1 : g.num0);
            bad = bad || (played && !ok);
            // one pass per member that finished a game in this wave, lane 0 adds the pass's counts (EVG_WINNER_P0 / P1 are the seats' numbers)
            uint64_t rest = __ballot(ok);
            while (rest) {
                const int mm = __builtin_amdgcn_readlane(m[p], __ffsll((unsigned long long)rest) - 1);
                const bool mine = ok && m[p] == mm;
                const uint64_t bm = __ballot(mine);
                const int ng = __popcll(bm), nw = __popcll(__ballot(mine && w == p)), nt = __popcll(__ballot(mine && w == EVG_WINNER_TIE));
                if (lane == 0) {
                    unsigned long long* const c = g.counts + 4 * (p * EVG_POP_MAX_MEMBERS + mm);
                    atomicAdd(&c[0], (unsigned long long)ng);
                    if (nw) atomicAdd(&c[1], (unsigned long long)nw);
                    if (nt) atomicAdd(&c[2], (unsigned long long)nt);
                    if (ng - nw - nt) atomicAdd(&c[3], (unsigned long long)(ng - nw - nt));
                }
                rest &= ~bm;
            }
        }
        if (bad) atomicOr(g.ctl, (unsigned long long)EVG_POP_S_BAD_MEMBER);
    }
    if (act) {
        g.member[2 * e] = (uint8_t)pop_draw(S, e, 0, g.num0);
        g.member[2 * e + 1] = (uint8_t)pop_draw(S, e, 1, g.num1);
    }
}

// ---- the bucket pass: rows -> per-member lists, a stable counting sort
struct PopBucket {
    const uint8_t* member;       // [rows][S]
    int32_t* index;              // [S][rows]
    int32_t* first;              // [S][POP_BINS]
    int32_t* count;              // [S][POP_BINS]
    int32_t* hist;               // [S][POP_BINS][nb]
    unsigned long long* ctl;
    float* out;                  // q_out: rows of row_floats floats at [(r * S + slot) * row_floats]
    int32_t rows, S, nb, row_floats;
    int32_t num0, num1;          // members of the team that plays seat slot 0 / 1
};

// the bin of row r of seat slot `slot` (-1: no such row), its wave's count of every bin -> wc[wave][bin], and the row's rank among its wave's rows of its bin
__device__ __forceinline__ int pop_rank(const PopBucket& b, int r, int slot, int* __restrict__ wc, int& bin) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bin = -1;
    if (r < b.rows) {
        const int id = b.member[(long long)r * b.S + slot];
        bin = id < (slot ? b.num1 : b.num0) ? id : EVG_POP_MAX_MEMBERS;
    }
    int rank = 0;
    for (int k = 0; k < POP_BINS; ++k) {
        const uint64_t mk = __ballot(bin == k);
        if (lane == 0) wc[wave * POP_BINS + k] = __popcll(mk);
        if (bin == k) rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    }
    return rank;
}

__global__ void __launch_bounds__(POP_BLOCK) evg_population_hist_kernel(PopBucket b) {
    __shared__ int wc[(POP_BLOCK / 64) * POP_BINS];
    const int slot = blockIdx.y;
    int bin;
    pop_rank(b, blockIdx.x * POP_BLOCK + threadIdx.x, slot, wc, bin);
    __syncthreads();
    if (threadIdx.x < POP_BINS) {
        int v = 0;
        for (int w = 0; w < POP_BLOCK / 64; ++w) v += wc[w * POP_BINS + threadIdx.x];
        b.hist[((long long)slot * POP_BINS + threadIdx.x) * b.nb + blockIdx.x] = v;
    }
}

// one workgroup per seat slot: per bin, the block counts -> each block's first position in the slot's list (in place); the bin's extent -> first / count
__global__ void __launch_bounds__(256) evg_population_scan_kernel(PopBucket b) {
    __shared__ int lds[4];
    const int slot = blockIdx.x;
    const int per = (b.nb + 255) / 256;
    const int lo = threadIdx.x * per < b.nb ? threadIdx.x * per : b.nb, hi = lo + per < b.nb ? lo + per : b.nb;
    int base = 0;
    for (int k = 0; k < POP_BINS; ++k) {
        int* const bs = b.hist + ((long long)slot * POP_BINS + k) * b.nb;
        int v = 0;
        for (int i = lo; i < hi; ++i) v += bs[i];
        int total;
        int run = base + rp_block_exclusive(v, lds, &total);
        for (int i = lo; i < hi; ++i) {
            const int x = bs[i];
            bs[i] = run;
            run += x;
        }
        if (threadIdx.x == 0) {
            b.first[slot * POP_BINS + k] = base;
            b.count[slot * POP_BINS + k] = total;
        }
        base += total;
    }
}

__global__ void __launch_bounds__(POP_BLOCK) evg_population_scatter_kernel(PopBucket b) {
    __shared__ int wc[(POP_BLOCK / 64) * POP_BINS];
    const int slot = blockIdx.y, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * POP_BLOCK + threadIdx.x;
    int bin;
    const int rank = pop_rank(b, r, slot, wc, bin);
    __syncthreads();
    if (bin < 0) return;
    int pos = b.hist[((long long)slot * POP_BINS + bin) * b.nb + blockIdx.x] + rank;
    for (int w = 0; w < wave; ++w) pos += wc[w * POP_BINS + bin];
    if ((unsigned)pos < (unsigned)b.rows) b.index[(long long)slot * b.rows + pos] = r;
    if (bin == EVG_POP_MAX_MEMBERS) {                 // no such member: zeros, and the status bit; the id selects nothing
        float* const o = b.out + ((long long)r * b.S + slot) * b.row_floats;
        for (int i = 0; i < b.row_floats; ++i) o[i] = 0.0f;
        atomicOr(b.ctl, (unsigned long long)EVG_POP_S_BAD_MEMBER);
    }
}

// ---- the grouped forward
struct MiniPopArgs {
    MiniQnetArgs q;                                   // (its `set` is not read: the sets are below)
    MiniQnetSet set[2][EVG_POP_MAX_MEMBERS];          // [seat slot][member]
    const int32_t* index;
    const int32_t* first;
    const int32_t* count;
    int32_t num0, num1, ky;                           // members per seat slot; blockIdx.y = slot * ky + member
};

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_mini_qnet_pop_kernel(MiniPopArgs p) {
    constexpr int WLDS = EXPANDED ? MQ_H * MQ_W1S : MQ_H * MQ_W1PS + 12 * MQ_H;
    __shared__ float wl[WLDS];
    __shared__ float tiles[QN_WAVES][16 * MQ_HS];
    const int slot = (int)blockIdx.y / p.ky, member = (int)blockIdx.y - slot * p.ky;
    if (member >= (slot ? p.num1 : p.num0)) return;
    // The grid is sized for the worst case (every row on one member): the counts live on the device.  A member's rows get its share of the grid's
    // workgroups -- what a plain launch over as many rows would run -- and the others leave here, uniformly, before any weight is staged.
    const long long rows = p.q.rows;
    long long cnt = p.count[slot * POP_BINS + member];
    cnt = cnt < rows ? cnt : rows;
    if (cnt <= 0) return;
    long long first = p.first[slot * POP_BINS + member];
    first = first < 0 ? 0 : (first < rows - cnt ? first : rows - cnt);
    const long long need = (cnt + 16 * QN_WAVES - 1) / (16 * QN_WAVES);
    long long live = ((long long)gridDim.x * cnt + rows - 1) / rows;
    live = live < need ? live : need;
    if ((long long)blockIdx.x >= live) return;
    const MiniQnetArgs& a = p.q;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = slot;
    const MiniQnetSet W = p.set[slot][member];
    const int* const list = p.index + (long long)slot * rows + first;
    const long long list_rows = cnt, list_stride = live * QN_WAVES;
#define MQ_GROUPED 1
#include "minimized_qnet_body.inc"
#undef MQ_GROUPED
}

// ---- the grouped Smart_State forward (evg_smart_population): evg_qnet_kernel with a workgroup belonging to one (seat slot, member)
struct SmartPopArgs {
    QnetArgs q;                                       // (its `set` is not read: the sets are below)
    QnetSet set[2][EVG_POP_MAX_MEMBERS];              // [seat slot][member]
    const int32_t* index;
    const int32_t* first;
    const int32_t* count;
    int32_t num0, num1, ky;                           // members per seat slot; blockIdx.y = slot * ky + member
};

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES) evg_qnet_pop_kernel(SmartPopArgs p) {
    __shared__ float fixed[QN_FIXED];
    __shared__ __attribute__((aligned(16))) float lds[QN_UNION];
    const int slot = (int)blockIdx.y / p.ky, member = (int)blockIdx.y - slot * p.ky;
    if (member >= (slot ? p.num1 : p.num0)) return;
    // evg_mini_qnet_pop_kernel's prologue: a member's rows get its share of a grid sized for the worst case, the other workgroups leave here, uniformly,
    // before any weight is staged
    const long long rows = p.q.rows;
    long long cnt = p.count[slot * POP_BINS + member];
    cnt = cnt < rows ? cnt : rows;
    if (cnt <= 0) return;
    long long first = p.first[slot * POP_BINS + member];
    first = first < 0 ? 0 : (first < rows - cnt ? first : rows - cnt);
    const long long need = (cnt + 16 * QN_WAVES - 1) / (16 * QN_WAVES);
    long long live = ((long long)gridDim.x * cnt + rows - 1) / rows;
    live = live < need ? live : need;
    if ((long long)blockIdx.x >= live) return;
    const QnetArgs& a = p.q;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seat = slot;
    const QnetSet W = p.set[slot][member];
    const int* const list = p.index + (long long)slot * rows + first;
    const long long list_rows = cnt, list_stride = live * QN_WAVES;
#define QN_GROUPED 1
#include "qnet_body.inc"
#undef QN_GROUPED
}

static PopArgs pop_args(const evg_population& pop) { return PopArgs{pop.member, pop.counts, pop.ctl, pop.num_members[0], pop.num_members[1]}; }

int launch_population_clear(const DevState& S, const evg_population& pop, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(pop.counts, 0, sizeof(unsigned long long) * 2 * EVG_POP_MAX_MEMBERS * 4, s) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(pop.ctl, 0, sizeof(unsigned long long) * 2, s) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(evg_population_clear_kernel, dim3((S.N + 255) / 256), dim3(256), 0, s, S, pop_args(pop));
    return (int)hipGetLastError();
}

int launch_population_assign(const DevState& S, const evg_population& pop, const uint8_t* mask, const int8_t* winner, uint8_t* history, void* stream) {
    hipLaunchKernelGGL(evg_population_assign_kernel, dim3((S.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), S, pop_args(pop), mask,
                       winner, history);
    return (int)hipGetLastError();
}

// the bucket pass of one call (three launches on s) and the grouped forward's arguments p; -> the forward's grid.  Shared by the fp32 launch below and
// the bf16 one (population_bf16_kernels.inc)
static dim3 population_qnet_prepare(const evg_population& pop, int layout, long long rows, int seat, const uint8_t* member, const float* in0,
                                    const float* in1, float* q_out, int num_cu, hipStream_t s, MiniPopArgs& p) {
    const int S = layout == EVG_QNET_COMPACT_SEATS ? 2 : 1;
    const int team[2] = {S == 2 ? 0 : seat, 1};      // the team that plays seat slot 0 / 1
    PopBucket b;
    b.member = member; b.index = pop.index; b.first = pop.first; b.count = pop.count; b.hist = pop.hist; b.ctl = pop.ctl; b.out = q_out;
    b.rows = (int32_t)rows; b.S = S; b.nb = (int32_t)((rows + POP_BLOCK - 1) / POP_BLOCK);
    b.row_floats = layout == EVG_QNET_EXPANDED ? MQ_OUT : 12 * MQ_OUT;
    b.num0 = pop.num_members[team[0]]; b.num1 = pop.num_members[team[1]];
    hipLaunchKernelGGL(evg_population_hist_kernel, dim3((unsigned)b.nb, (unsigned)S), dim3(POP_BLOCK), 0, s, b);
    hipLaunchKernelGGL(evg_population_scan_kernel, dim3((unsigned)S), dim3(256), 0, s, b);
    hipLaunchKernelGGL(evg_population_scatter_kernel, dim3((unsigned)b.nb, (unsigned)S), dim3(POP_BLOCK), 0, s, b);

    for (int t = 0; t < 2; ++t) p.q.set[t] = MiniQnetSet{nullptr, nullptr, nullptr, nullptr};
    p.q.h1 = pop.h1; p.q.final_relu = pop.final_relu; p.q.num_seats = S; p.q.rows = rows; p.q.in0 = in0; p.q.in1 = in1; p.q.out = q_out;
    for (int t = 0; t < 2; ++t)
        for (int m = 0; m < EVG_POP_MAX_MEMBERS; ++m) {
            const int q = team[t];
            p.set[t][m] = m < pop.num_members[q] ? MiniQnetSet{pop.w1[q][m], pop.b1[q][m], pop.w2[q][m], pop.b2[q][m]} : MiniQnetSet{nullptr, nullptr, nullptr, nullptr};
        }
    p.index = pop.index; p.first = pop.first; p.count = pop.count;
    p.num0 = b.num0; p.num1 = b.num1;
    p.ky = S == 2 && b.num1 > b.num0 ? b.num1 : b.num0;
    // the plain launch's grid (two workgroups per CU resident) per seat slot, times the members: each member's rows use their share of it
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)blocks, (unsigned)(S * p.ky));
}

int launch_population_qnet(const evg_population& pop, int layout, long long rows, int seat, const uint8_t* member, const float* in0, const float* in1,
                           float* q_out, int num_cu, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MiniPopArgs p;
    const dim3 grid = population_qnet_prepare(pop, layout, rows, seat, member, in0, in1, q_out, num_cu, s, p);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_mini_qnet_pop_kernel<true>, grid, dim3(64 * QN_WAVES), 0, s, p);
    else
        hipLaunchKernelGGL(evg_mini_qnet_pop_kernel<false>, grid, dim3(64 * QN_WAVES), 0, s, p);
    return (int)hipGetLastError();
}

static PopArgs pop_args(const evg_smart_population& pop) { return PopArgs{pop.member, pop.counts, pop.ctl, pop.num_members[0], pop.num_members[1]}; }

// the assignment of a Smart_State population: the same two kernels through the same PopArgs, hence the same draws
int launch_smart_population_clear(const DevState& S, const evg_smart_population& pop, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(pop.counts, 0, sizeof(unsigned long long) * 2 * EVG_POP_MAX_MEMBERS * 4, s) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(pop.ctl, 0, sizeof(unsigned long long) * 2, s) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(evg_population_clear_kernel, dim3((S.N + 255) / 256), dim3(256), 0, s, S, pop_args(pop));
    return (int)hipGetLastError();
}

int launch_smart_population_assign(const DevState& S, const evg_smart_population& pop, const uint8_t* mask, const int8_t* winner, uint8_t* history,
                                   void* stream) {
    hipLaunchKernelGGL(evg_population_assign_kernel, dim3((S.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), S, pop_args(pop), mask,
                       winner, history);
    return (int)hipGetLastError();
}

// population_qnet_prepare for the Smart_State network
static dim3 smart_population_qnet_prepare(const evg_smart_population& pop, int layout, long long rows, int seat, const uint8_t* member, const float* in0,
                                          const float* in1, float* q_out, int num_cu, hipStream_t s, SmartPopArgs& p) {
    const int S = layout == EVG_QNET_COMPACT_SEATS ? 2 : 1;
    const int team[2] = {S == 2 ? 0 : seat, 1};      // the team that plays seat slot 0 / 1
    PopBucket b;
    b.member = member; b.index = pop.index; b.first = pop.first; b.count = pop.count; b.hist = pop.hist; b.ctl = pop.ctl; b.out = q_out;
    b.rows = (int32_t)rows; b.S = S; b.nb = (int32_t)((rows + POP_BLOCK - 1) / POP_BLOCK);
    b.row_floats = layout == EVG_QNET_EXPANDED ? QN_OUT : 12 * QN_OUT;
    b.num0 = pop.num_members[team[0]]; b.num1 = pop.num_members[team[1]];
    hipLaunchKernelGGL(evg_population_hist_kernel, dim3((unsigned)b.nb, (unsigned)S), dim3(POP_BLOCK), 0, s, b);
    hipLaunchKernelGGL(evg_population_scan_kernel, dim3((unsigned)S), dim3(256), 0, s, b);
    hipLaunchKernelGGL(evg_population_scatter_kernel, dim3((unsigned)b.nb, (unsigned)S), dim3(POP_BLOCK), 0, s, b);

    for (int t = 0; t < 2; ++t) p.q.set[t] = QnetSet{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    p.q.h1 = pop.h1; p.q.h2 = pop.h2; p.q.final_relu = pop.final_relu; p.q.num_seats = S; p.q.rows = rows; p.q.in0 = in0; p.q.in1 = in1; p.q.out = q_out;
    for (int t = 0; t < 2; ++t)
        for (int m = 0; m < EVG_POP_MAX_MEMBERS; ++m) {
            const int q = team[t];
            p.set[t][m] = m < pop.num_members[q] ? QnetSet{pop.w1[q][m], pop.b1[q][m], pop.w2[q][m], pop.b2[q][m], pop.w3[q][m], pop.b3[q][m]}
                                                 : QnetSet{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        }
    p.index = pop.index; p.first = pop.first; p.count = pop.count;
    p.num0 = b.num0; p.num1 = b.num1;
    p.ky = S == 2 && b.num1 > b.num0 ? b.num1 : b.num0;
    // launch_smart_qnet's grid (two workgroups per CU resident) per seat slot, times the members: each member's rows use their share of it
    const long long groups = (rows + 15) / 16;
    long long blocks = (groups + QN_WAVES - 1) / QN_WAVES;
    const long long cap = 2LL * (num_cu > 0 ? num_cu : 256);
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)blocks, (unsigned)(S * p.ky));
}

int launch_smart_population_qnet(const evg_smart_population& pop, int layout, long long rows, int seat, const uint8_t* member, const float* in0,
                                 const float* in1, float* q_out, int num_cu, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SmartPopArgs p;
    const dim3 grid = smart_population_qnet_prepare(pop, layout, rows, seat, member, in0, in1, q_out, num_cu, s, p);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_qnet_pop_kernel<true>, grid, dim3(64 * QN_WAVES), 0, s, p);
    else
        hipLaunchKernelGGL(evg_qnet_pop_kernel<false>, grid, dim3(64 * QN_WAVES), 0, s, p);
    return (int)hipGetLastError();
}
