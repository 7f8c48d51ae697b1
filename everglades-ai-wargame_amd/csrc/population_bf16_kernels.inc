// population_bf16_kernels.inc -- self-royale on the bf16 matrix cores (include/evg_pop_bf16.h: evg_population_qnet_bf16, evg_smart_population_qnet_bf16):
// the grouped forward of population_kernels.inc with the bodies of qnet_bf16_kernels.inc.  Included by evg_kernels.hip (namespace evg) under EVG_POP_BF16
// (with EVG_BF16: `make popbf16`, libevg_popbf16.so), after both of them; neither is touched.
//
//   evg_qnet_pop_bf16_kernel<EXPANDED>        evg_qnet_bf16_kernel (qnet_bf16_body.inc) with a workgroup belonging to one (seat slot, member)
//   evg_mini_qnet_pop_bf16_kernel<EXPANDED>   evg_mini_qnet_bf16_kernel (minimized_qnet_bf16_body.inc), the same
//
// The bucket pass (evg_population_hist / _scan / _scatter_kernel) is population_kernels.inc's own, unchanged: the lists, first / count and the zeros
// and status bit of the rows of nobody are what the fp32 call publishes.  The prologue is the fp32 grouped kernels': blockIdx.y = slot * ky + member, a
// member's rows get their share of a grid sized for the worst case, and the other workgroups leave uniformly before any weight is staged.
//
// Rows.  In the bf16 orientation a lane's results are those of its own row (column n of every tile), so ONE list entry per lane names where the lane
// reads and where it writes; the fp32 kernels need the four rows of a D fragment besides.  A lane past the end of the list takes the list's last entry
// and stores nothing.  Every MFMA column depends on that column of B alone and the instruction sequence per row is the shared body, so a row's Q equals,
// bit for bit, what the plain bf16 kernel writes for it with the member's weights.
//
// Both kernels ask for two workgroups per CU (2 wavefronts per SIMD: at most 256 registers), which the plain compact kernels have.

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES, 2) evg_qnet_pop_bf16_kernel(SmartPopArgs p) {
    constexpr int L1F = EXPANDED ? 8 : 12;                // evg_qnet_bf16_kernel's LDS
    __shared__ qb_bf8 w1s[L1F * 64], w2s[8 * 64], w3s[2 * 64];
    const int slot = (int)blockIdx.y / p.ky, member = (int)blockIdx.y - slot * p.ky;
    if (member >= (slot ? p.num1 : p.num0)) return;
    // evg_mini_qnet_pop_kernel's prologue
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
#define QB_GROUPED 1
#include "qnet_bf16_body.inc"
#undef QB_GROUPED
}

template <bool EXPANDED>
__global__ void __launch_bounds__(64 * QN_WAVES, 2) evg_mini_qnet_pop_bf16_kernel(MiniPopArgs p) {
    constexpr int L1F = EXPANDED ? 2 * MQ_TILES : 3 * MQ_TILES;      // evg_mini_qnet_bf16_kernel's LDS
    __shared__ qb_bf8 w1s[L1F * 64], w2s[(MQ_TILES / 2) * 64];
    __shared__ __attribute__((aligned(16))) float b1s[MQ_H];
    const int slot = (int)blockIdx.y / p.ky, member = (int)blockIdx.y - slot * p.ky;
    if (member >= (slot ? p.num1 : p.num0)) return;
    // evg_mini_qnet_pop_kernel's prologue
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
#define QB_GROUPED 1
#include "minimized_qnet_bf16_body.inc"
#undef QB_GROUPED
}

int launch_population_qnet_bf16(const evg_population& pop, int layout, long long rows, int seat, const uint8_t* member, const float* in0,
                                const float* in1, float* q_out, int num_cu, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MiniPopArgs p;
    const dim3 grid = population_qnet_prepare(pop, layout, rows, seat, member, in0, in1, q_out, num_cu, s, p);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_mini_qnet_pop_bf16_kernel<true>, grid, dim3(64 * QN_WAVES), 0, s, p);
    else
        hipLaunchKernelGGL(evg_mini_qnet_pop_bf16_kernel<false>, grid, dim3(64 * QN_WAVES), 0, s, p);
    return (int)hipGetLastError();
}

int launch_smart_population_qnet_bf16(const evg_smart_population& pop, int layout, long long rows, int seat, const uint8_t* member, const float* in0,
                                      const float* in1, float* q_out, int num_cu, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SmartPopArgs p;
    const dim3 grid = smart_population_qnet_prepare(pop, layout, rows, seat, member, in0, in1, q_out, num_cu, s, p);
    if (layout == EVG_QNET_EXPANDED)
        hipLaunchKernelGGL(evg_qnet_pop_bf16_kernel<true>, grid, dim3(64 * QN_WAVES), 0, s, p);
    else
        hipLaunchKernelGGL(evg_qnet_pop_bf16_kernel<false>, grid, dim3(64 * QN_WAVES), 0, s, p);
    return (int)hipGetLastError();
}
