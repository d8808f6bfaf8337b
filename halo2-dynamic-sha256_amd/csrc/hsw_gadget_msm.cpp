// hsw_gadget_msm.cpp -- the commitments of device columns (include/hsw.h, "commit device columns"): every refusal decided
// on the host, the plan of hsw_msm_value.hpp, the launches of hsw_msm.hip group of columns by group, then the host tail
// -- W window points per column copied back, the Horner over the windows and the one inversion, with the value layer's
// own code.  A translation unit of its own: only the entry point below refers to those kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

#include "hsw_msm.h"
#include "hsw_nounwind.hpp"

namespace {

const size_t MSM_GRID_COLUMNS = 65535;                         // blockIdx.z, blockIdx.y

using hsw::fail_at;

}  // namespace

extern "C" int hsw_gadget_msm(hsw_gadget *g, const hsw_msm *args, hsw_msm_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->first_refused = report->first_bad_base = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const size_t n = args->n_columns;
    if (n == 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_columns is at least 1");
    if (args->flags) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    if (args->n_bases < 1 || args->n_bases > (1ull << hsw::MSM_MAX_LOG_BASES)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_bases is 1 .. 2^28");
    const uintptr_t bases = reinterpret_cast<uintptr_t>(args->d_bases);
    if (!bases || (bases & 15u)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "d_bases is NULL or not 16-byte aligned");
    if (!args->d_scalars) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "the column pointer array is NULL");
    if (!args->out_points) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "out_points is NULL");
    uint64_t max_rows = 0;
    for (size_t b = 0; b < n; b++) {
        const uint64_t rows = args->input_rows ? args->input_rows[b] : args->n_bases;
        if (rows > args->n_bases) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "input_rows above n_bases");
        const uintptr_t in = reinterpret_cast<uintptr_t>(args->d_scalars[b]);
        if (!in || (in & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "a scalar pointer that is NULL or not 16-byte aligned");
        max_rows = std::max(max_rows, rows);
    }
    hsw::MsmPlan plan;
    if (!hsw::msm_plan((uint32_t)max_rows, args->window_bits, args->slice_rows, plan))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "window_bits is 0 .. 8 and slice_rows 0 or a power of two, 64 .. 2^28");
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    // columns in groups whose partial buckets fit the scratch (1 GiB, or what the option "round_scratch" lowers it to); the
    // grid limit cannot be the one that cuts: at one bucket per window a column still takes 24 KB, 65,535 of them above 1 GiB
    const size_t column_bytes = (size_t)hsw::msm_partial_points(plan) * sizeof(hsw::G1);
    const size_t group = std::min(std::min(n, MSM_GRID_COLUMNS), std::max<size_t>(1, e->round_scratch / column_bytes));
    const size_t n_groups = (n + group - 1) / group;
    // device staging: [status words][the bases' check][columns][window points][partial buckets of a group]
    const hsw::MsmCheck check0{0u, ~0u};
    hsw::Staging st;
    st.zeroed(n * sizeof(uint32_t));
    const size_t off_check = st.add(&check0, sizeof check0), off_cols = st.zeroed(n * sizeof(hsw::MsmColumn));
    const size_t win_bytes = n * plan.windows * sizeof(hsw::G1), off_win = st.work(win_bytes);
    const size_t scratch_bytes = group * column_bytes, off_partial = st.work(scratch_bytes);
    for (size_t b = 0; b < n; b++) {
        hsw::MsmColumn &mc = st.image<hsw::MsmColumn>(off_cols)[b];
        mc.cells = static_cast<const uint4 *>(args->d_scalars[b]);
        mc.rows = (uint32_t)(args->input_rows ? args->input_rows[b] : args->n_bases);
    }
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    hsw::MsmParams p{};
    p.plan = plan;
    p.bases = static_cast<const uint4 *>(args->d_bases);
    p.partial = hsw::at<uint4>(d, off_partial);
    p.montgomery = mont ? 1u : 0u;
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    if (he == hipSuccess) he = hsw::launch_msm_check(p.bases, (uint32_t)max_rows, hsw::at<hsw::MsmCheck>(d, off_check), stream);
    for (size_t b0 = 0; he == hipSuccess && b0 < n; b0 += group) {
        const uint32_t cols = (uint32_t)std::min(group, n - b0);
        p.cols = hsw::at<const hsw::MsmColumn>(d, off_cols) + b0;
        p.status = hsw::at<uint32_t>(d, 0) + b0;
        p.windows = hsw::at<uint4>(d, off_win + b0 * plan.windows * sizeof(hsw::G1));
        he = hsw::launch_msm_accumulate(p, cols, stream);
        if (he == hipSuccess) he = hsw::launch_msm_reduce(p, cols, stream);
    }
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint8_t> back(off_cols + win_bytes);         // the status words and the check, then the window points
    if (he == hipSuccess) he = hipMemcpyAsync(back.data() + off_cols, hsw::at<uint8_t>(d, off_win), win_bytes, hipMemcpyDeviceToHost, stream);
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, back.data(), off_cols, ms);
    if (frc != HSW_OK) return frc;
    const auto t0 = std::chrono::steady_clock::now();
    hsw::MsmCheck check;
    std::memcpy(&check, back.data() + off_check, sizeof check);
    const uint32_t *status = reinterpret_cast<const uint32_t *>(back.data());
    std::vector<hsw::G1> win(plan.windows);
    for (size_t b = 0; b < n; b++) {
        const uint32_t st = (status[b] & hsw::MSM_CELL_NOT_BELOW_P) | (check.bad ? (uint32_t)hsw::MSM_BASE_NOT_BELOW_Q : 0u);
        if (st) { if (!report->refused_columns++) report->first_refused = b; }
        else {
            std::memcpy(win.data(), back.data() + off_cols + b * plan.windows * sizeof(hsw::G1), plan.windows * sizeof(hsw::G1));
            const hsw::G1Affine out = hsw::msm_normalise(hsw::msm_horner(win.data(), plan.windows, plan.window_bits));
            std::memcpy(static_cast<uint8_t *>(args->out_points) + b * sizeof out, &out, sizeof out);
        }
        if (args->status) args->status[b] = st;
    }
    report->finish_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    report->kernel_ms = ms[0];
    report->columns = n;
    report->bad_bases = check.bad;
    if (check.bad) report->first_bad_base = check.first;
    report->scratch_bytes = scratch_bytes;
    report->window_bits = plan.window_bits;
    report->windows = plan.windows;
    report->slice_rows = plan.slice_rows;
    report->slices = plan.slices;
    report->launches = (uint32_t)((max_rows ? 1 : 0) + 2 * n_groups);
    return HSW_OK;
} HSW_NO_UNWIND
