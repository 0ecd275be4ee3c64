// The chunk loop of Separator.forward (/root/reference/xumx_slicq_v2/separator.py:133-232) issued from native code:
// one C call enqueues every launch of a track -- stacked full chunks on the caller's stream, the short tail chunk on a
// side stream beside them -- through row-offset tables cached per call shape.  No kernels of its own: it sequences
// the entry points of slicqt.hip / cdae.hip / wiener.hip (include/xumx_slicq_hip.h, "the whole call").
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "cdae_api.h"
#include "common.h"
#include "plan.h"
#include "xumx_slicq_hip.h"

using namespace xsq;

namespace {

// what the 32-bit float offsets of the band kernels allow for the 8-channel estimate arena of one pass:
// 2 * (8 B) * S * sumFT < 2^31 (slicqt.hip: inverse_impl) -> B * S <= 7168 for the Bark-262 plan (sumFT = 18640)
// (J sources: 2J channels per sample; 4 without the residual of xsq_model_set_wiener_options)
// (coefs complex coefficients per channel-slice, floor = the L / 2 + 1 spectrum bins of a slice)
static int default_max_item_slices(int64_t coefs, int64_t floor, int J = 4) {
    const int64_t lim = ((1ll << 31) - 1) / (4 * J * std::max<int64_t>(coefs, floor));
    return (int)std::min<int64_t>(lim, 65535 / (2 * J));    // and BC * S <= 65535 rows per launch
}
static int default_max_item_slices(const xsq_plan* P, int J = 4) { return default_max_item_slices(P->sumFT, P->nbins, J); }

static inline int sources_of(const xsq_model* Mo) { return (Mo->wiener_flags & XSQ_WIENER_RESIDUAL) ? 5 : 4; }

struct PassPlan {
    int64_t n = 0, n_pad = 0;        // samples per item that exist / that the slice count is taken from
    int B = 0, group = 1;            // stacked items (chunk, sample); samples per chunk in this pass
    int tail = 0;                    // 1: runs on the tail stream
    // a batch split over several passes under Wiener-EM: the passes of one chunk range (a "set") share a table of window
    // maxima taken over ALL their samples (norbert/__init__.py:257 spans the batch) -- float offset into the table buffer at
    // the head of the workspace, -1 = none; set_first / set_count: the passes of the set (consecutive)
    int64_t ext_off = -1;
    int set_first = 0, set_count = 1;
    const int64_t* d_xrows = nullptr;      // [2B] input row offsets (null: rows one after the other)
    const int64_t* d_orows = nullptr;      // [2JB] output row offsets (J = 4 sources, 5 with the residual)
    // a pass of overlapped segments (xsq_separator_forward_segments): d_orows point into the scratch arena and one
    // xsq_crossfade_place launch blends the seg_k segments at seg_start + j * seg_stride into the result
    int64_t seg_start = 0, seg_stride = 0;
    int seg_k = 0, fade_in = 0, fade_out = 0;
};

struct ForwardPlan {
    std::vector<PassPlan> passes;
    int64_t* d_tables = nullptr;     // one allocation behind all d_xrows / d_orows
    int64_t* h_tables = nullptr;     // pinned host copy: uploaded when the plan is made, on the demixer's own copy stream (no device-wide stall)
    size_t table_words = 0;
    bool pinned = false;             // a HIP graph captured a call of this shape: its nodes hold d_xrows / d_orows, never evicted
    uint64_t last_use = 0;           // LRU stamp (xsq_demixer::clock)
    size_t main_bytes = 0, tail_bytes = 0;
    size_t ext_floats = 0;           // window-maximum tables of the split sets (zeroed at the start of every call)
    size_t scratch_bytes = 0;        // overlapped segments: the un-faded stems of the largest pass (head of the workspace)
};

}  // namespace

struct xsq_demixer {
    xsq_plan* plan = nullptr;
    int max_item_slices = 0;
    std::vector<int32_t> F, T;
    std::mutex mu;
    // schedules + device row tables per call shape, least-recently-used bound: a test set of distinct track lengths would
    // otherwise leave one device allocation per length behind
    std::map<std::vector<int64_t>, ForwardPlan> plans;
    uint64_t clock = 0;
    static constexpr size_t kMaxPlans = 64;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t up_stream = nullptr;     // row-table uploads: a non-blocking stream of its own, waited for on the host per NEW shape
};

namespace {

struct PassLayout {
    size_t X, masks, Y, fwd, cdae, inv, wien, total;
    size_t fwd_bytes, cdae_bytes, inv_bytes, wien_bytes;
};

// workspace of one pass: X arena | masks arena | [Y arena] | forward ws | CDAE ws | inverse ws | [Wiener ws]
static int pass_layout(xsq_demixer* d, const xsq_model* Mo, int B, int64_t n_pad, int wiener, PassLayout* L) {
    xsq_plan* P = d->plan;
    const int S = xsq_plan_num_slices(P, n_pad);
    XSQ_REQUIRE(S >= 3, "xsq_demix_pass: %lld samples give %d slices; the conv stack needs 3 (pad to sllen/2 + 1)", (long long)n_pad, S);
    XSQ_REQUIRE(Mo->sumFT == P->sumFT && Mo->nblocks == P->nblocks, "xsq_demix_pass: the model's block table is not the plan's");
    const size_t coefs = (size_t)S * P->sumFT;
    const int flags = Mo->wiener_flags, J = sources_of(Mo);
    size_t o = 0;
    L->X = o;     o += al256((size_t)2 * B * coefs * 8);
    L->masks = o; o += al256((size_t)8 * B * coefs * 4);
    L->Y = o;     if (wiener || flags) o += al256((size_t)2 * J * B * coefs * 8);
    L->fwd_bytes = xsq_slicqt_forward_workspace(P, 2 * B, n_pad);
    L->cdae_bytes = xsq_cdae_workspace(Mo, B, S);
    L->inv_bytes = xsq_slicqt_inverse_workspace(P, 2 * J * B, S);
    L->wien_bytes = flags ? xsq_wiener_options_workspace(P->nblocks, d->F.data(), d->T.data(), B, S, 5000, wiener, 0, flags)
                  : wiener >= 2 ? xsq_wiener_iter_workspace(P->nblocks, d->F.data(), d->T.data(), B, S, 5000, wiener, 0)
                  : wiener ? xsq_wiener_workspace(P->nblocks, d->F.data(), d->T.data(), B, S, 5000) : 0;
    if (!L->fwd_bytes || !L->cdae_bytes || !L->inv_bytes || ((wiener || flags) && !L->wien_bytes)) {
        const std::string why = xsq_last_error();
        set_error("xsq_demix_pass: B=%d, %lld samples: a stage's workspace query failed (%s)", B, (long long)n_pad, why.c_str());
        return XSQ_ERR_ARG;
    }
    L->fwd = o;  o += al256(L->fwd_bytes);
    L->cdae = o; o += al256(L->cdae_bytes);
    L->inv = o;  o += al256(L->inv_bytes);
    L->wien = o; o += al256(L->wien_bytes);
    L->total = o + 256;
    return XSQ_OK;
}

// The remix tail of a pass (xsq_separator_remix): the mixes two at a time through xsq_slicqt_inverse_remix, in the space
// behind the inverse transform's own workspace -- free once the CDAE and the EM iterations are done.  Two mixes need at
// most the weighted arena of 4B channels plus the inverse workspace of 4B rows, which fits where the forward call's
// inverse of 8B rows runs: the forward call's workspace serves every R <= 4.  Output channel (r, item, c) is row
// (target = r, item, c) of the forward call's table.
static int run_remix(xsq_plan* P, const float* masks, const float* X, const float* Y, const float* gains, int R, int B, int S,
                     int64_t n, float* out, const int64_t* out_rows, void* ws, size_t ws_bytes, hipStream_t stream) {
    for (int r0 = 0; r0 < R; r0 += 2) {
        const int g = std::min(2, R - r0);
        if (int rc = xsq_slicqt_inverse_remix(P, masks, X, Y, gains + 4 * r0, g, B, S, n, out, out_rows + (size_t)r0 * 2 * B, ws,
                                              ws_bytes, stream))
            return rc;
    }
    return XSQ_OK;
}

// The input of a call: the audio itself, or a device slot that holds its address (xsq_separator_forward_indirect).
struct PassInput { const float* x; const float* const* x_slot; };

// One pass: of `p` this reads d_xrows / d_orows, B, n, n_pad and group.
static int run_pass(xsq_demixer* d, xsq_model* Mo, PassInput in, const PassPlan& p, int wiener, float* out, void* ws, size_t ws_bytes,
                    hipStream_t stream, const float* ext_max = nullptr, const float* gains = nullptr, int R = 0) {
    xsq_plan* P = d->plan;
    const int64_t n = p.n, n_pad = p.n_pad;
    const int B = p.B, group = p.group;
    PassLayout L;
    int rc = pass_layout(d, Mo, B, n_pad, wiener, &L);
    if (rc) return rc;
    if (L.total > ws_bytes) {
        set_error("xsq_demix_pass: workspace too small (%zu needed, %zu given)", L.total, ws_bytes);
        return XSQ_ERR_WORKSPACE;
    }
    const int S = xsq_plan_num_slices(P, n_pad);
    char* w = (char*)ws;
    float* X = (float*)(w + L.X);
    float* masks = (float*)(w + L.masks);
    float* Y = (float*)(w + L.Y);
    const float *mean, *scale;
    int split;
    if ((rc = xsq_model_whitening(Mo, &mean, &scale, &split))) return rc;
    // the analysis kernels write the whitened magnitude into the head of the CDAE workspace (xsq_cdae_forward_xin, xin_ready)
    float* xin = (float*)(w + L.cdae);
    if ((rc = xsq_slicqt_forward_rows_indirect(P, in.x, in.x_slot, p.d_xrows, 2 * B, n, n_pad, X, xin, mean, scale, split, w + L.fwd, L.fwd_bytes, stream)))
        return rc;
    if ((rc = xsq_cdae_forward_xin(Mo, X, B, S, nullptr, masks, w + L.cdae, L.cdae_bytes, stream, 1))) return rc;
    const int flags = Mo->wiener_flags, J = sources_of(Mo);
    if (flags) {
        // an option set (softmask, residual): J sources from the masks, whatever the iteration count; none writes the starts
        XSQ_REQUIRE(!gains || J == 4, "xsq_separator_remix: the residual has no gain column; remix the four targets without it");
        if ((rc = xsq_wiener_em_masked_options(P->nblocks, d->F.data(), d->T.data(), X, masks, Y, B, S, 5000, group, ext_max, wiener, 0, flags,
                                               w + L.wien, L.wien_bytes, stream)))
            return rc;
        if (!gains) return xsq_slicqt_inverse_rows(P, Y, 2 * J * B, S, n, out, p.d_orows, w + L.inv, L.inv_bytes, stream);
        return run_remix(P, nullptr, nullptr, Y, gains, R, B, S, n, out, p.d_orows, w + L.inv, L.total - L.inv, stream);
    }
    if (!wiener && !gains)
        return xsq_slicqt_inverse_masked(P, masks, X, 8 * B, 2 * B, S, n, out, p.d_orows, w + L.inv, L.inv_bytes, stream);
    // `wiener` counts the EM iterations: one runs the three launches it always ran, more take the form xsq_wiener_em_masked_iter
    // chooses (the window-resident kernel: 5000 frames fit)
    if (wiener == 1 && (rc = xsq_wiener_em_masked_ext(P->nblocks, d->F.data(), d->T.data(), X, masks, Y, B, S, 5000, group, ext_max,
                                                      w + L.wien, L.wien_bytes, stream)))
        return rc;
    if (wiener >= 2 && (rc = xsq_wiener_em_masked_iter(P->nblocks, d->F.data(), d->T.data(), X, masks, Y, B, S, 5000, group, ext_max,
                                                       wiener, 0, w + L.wien, L.wien_bytes, stream)))
        return rc;
    if (!gains) return xsq_slicqt_inverse_rows(P, Y, 8 * B, S, n, out, p.d_orows, w + L.inv, L.inv_bytes, stream);
    return run_remix(P, wiener ? nullptr : masks, wiener ? nullptr : X, wiener ? Y : nullptr, gains, R, B, S, n, out, p.d_orows,
                     w + L.inv, L.total - L.inv, stream);
}

// One pass of a split batch, first half: its mix transform and the window maxima of its samples folded into the set's table.
static int run_prepass(xsq_demixer* d, xsq_model* Mo, PassInput in, const PassPlan& p, void* ws, size_t ws_bytes, float* ext, hipStream_t stream) {
    xsq_plan* P = d->plan;
    PassLayout L;
    int rc = pass_layout(d, Mo, p.B, p.n_pad, 1, &L);
    if (rc) return rc;
    XSQ_REQUIRE(L.total <= ws_bytes, "xsq_separator_forward: workspace too small");
    const int S = xsq_plan_num_slices(P, p.n_pad);
    char* w = (char*)ws;
    float* X = (float*)(w + L.X);
    if ((rc = xsq_slicqt_forward_rows_indirect(P, in.x, in.x_slot, p.d_xrows, 2 * p.B, p.n, p.n_pad, X, nullptr, nullptr, nullptr, 0, w + L.fwd, L.fwd_bytes,
                                               stream)))
        return rc;
    return xsq_wiener_window_max(P->nblocks, d->F.data(), d->T.data(), X, p.B, S, 5000, p.group, ext + p.ext_off, stream);
}

// ---- the schedule of one call shape, pure host arithmetic (no device call: tests/test_abi_cpu.py drives it through
// xsq_separator_schedule): stacked passes over the full chunks (at most max_stack (chunk, sample) pairs and `cap`
// item-slices per pass), then the remaining chunks one by one (the tail passes); a batch too large for one pass is split
// over sample ranges, and under Wiener-EM the passes of such a set share a table of window maxima.
struct SchedPass {
    int64_t start, n;        // first sample of the first chunk of the pass; samples per chunk that exist
    int k, b0, nbb;          // chunks stacked, first sample index, samples
    int tail;                // 1: may run on the tail stream
    int set_first, set_count;
    int needs_ext;           // 1: the set shares a window-maximum table (Wiener-EM, set_count > 1)
};

static inline int64_t slices_of(int64_t n, int h) { return ((n + h - 1) / h + 1) / 2 + 1; }      // nsgt/slicing.py:47-72 (64 bits: chunk_size may be "none")

static void build_schedule(int L, int nb, int64_t N, int64_t cs, int max_stack, int wiener, int cap, std::vector<SchedPass>* out) {
    const int h = L / 4;
    const int64_t min_samples = L / 2 + 1;                         // separator.py:162
    auto close_set = [&](size_t first) {
        const int count = (int)(out->size() - first);
        for (size_t i = first; i < out->size(); ++i) {
            (*out)[i].set_first = (int)first; (*out)[i].set_count = count; (*out)[i].needs_ext = (wiener && count > 1) ? 1 : 0;
        }
    };
    const int64_t full = N / cs;
    const int S_full = (int)slices_of(std::max(cs, min_samples), h);
    // samples per pass: the whole batch when one chunk of it fits a launch, else the largest share that does
    const int nbb_max = std::max(1, std::min(nb, cap / std::max(1, S_full)));
    const int per_pass = (int)std::max<int64_t>(1, std::min<int64_t>(max_stack / std::max(1, nbb_max), cap / ((int64_t)nbb_max * S_full)));
    int64_t start = 0;
    while (full - start / cs >= 2 && per_pass >= 2) {
        const int k = (int)std::min<int64_t>(per_pass, full - start / cs);
        const size_t first = out->size();
        for (int b0 = 0; b0 < nb; b0 += nbb_max) out->push_back(SchedPass{start, cs, k, b0, std::min(nbb_max, nb - b0), 0, 0, 1, 0});
        close_set(first);
        start += (int64_t)k * cs;
    }
    const bool stacked = !out->empty();
    for (; start < N; start += cs) {
        const int64_t n = std::min(cs, N - start);
        const int S_n = (int)slices_of(std::max(n, min_samples), h);     // the sample split of a short chunk follows its own slice count
        const int nbb_n = std::max(1, std::min(nb, cap / std::max(1, S_n)));
        const size_t first = out->size();
        for (int b0 = 0; b0 < nb; b0 += nbb_n) out->push_back(SchedPass{start, n, 1, b0, std::min(nbb_n, nb - b0), stacked ? 1 : 0, 0, 1, 0});
        close_set(first);
    }
    bool any_ext = false;
    for (const SchedPass& p : *out) any_ext = any_ext || p.needs_ext;
    if (any_ext)                             // split sets under Wiener-EM run in order on the caller's stream
        for (SchedPass& p : *out) p.tail = 0;
}

// Room for one more call shape: when the cache is full the least recently used shape goes.  Its tables may still be read
// by kernels in flight (any stream): wait for the device once -- this happens once per kMaxPlans NEW shapes, never in a
// steady loop over known shapes.  Shapes a HIP graph has captured are never victims (a replay reads the tables without
// coming through here: ADVICE round 5); when every cached shape is pinned the cache simply grows.
static int evict_for_new_plan(xsq_demixer* d) {
    if (d->plans.size() < xsq_demixer::kMaxPlans) return XSQ_OK;
    auto victim = d->plans.end();
    for (auto p = d->plans.begin(); p != d->plans.end(); ++p)
        if (!p->second.pinned && (victim == d->plans.end() || p->second.last_use < victim->second.last_use)) victim = p;
    if (victim != d->plans.end()) {
        XSQ_HIP(hipDeviceSynchronize());
        (void)hipFree(victim->second.d_tables);
        (void)hipHostFree(victim->second.h_tables);
        d->plans.erase(victim);
    }
    return XSQ_OK;
}

// A plan while it is built: the passes, their row tables still on the host.
struct PlanBuild {
    ForwardPlan fp;
    std::vector<int64_t> rows;          // the row tables of the passes, one after the other
    // One more pass (B, group, n, ... set by the caller), its items (stacked chunk or segment j, sample b) = j * group + b:
    // channel c of an item is read at row x_of(item, c), source t of it is written at row o_of(t, item, c).
    template <class XOf, class OOf> void add_pass(const PassPlan& p, int J, XOf x_of, OOf o_of) {
        const size_t x0 = rows.size(), o0 = x0 + (size_t)2 * p.B;        // [2B] input rows, then [2JB] output rows
        rows.resize(o0 + (size_t)2 * J * p.B);
        for (int item = 0; item < p.B; ++item)
            for (int c = 0; c < 2; ++c) {
                rows[x0 + (size_t)item * 2 + c] = x_of(item, c);
                for (int t = 0; t < J; ++t) rows[o0 + ((size_t)t * p.B + item) * 2 + c] = o_of(t, item, c);
            }
        fp.passes.push_back(p);
    }
};

// The plan of a known call shape, stamped as used now.
static bool cached_plan(xsq_demixer* d, const std::vector<int64_t>& key, ForwardPlan** out) {
    auto it = d->plans.find(key);
    if (it == d->plans.end()) return false;
    it->second.last_use = ++d->clock;
    *out = &it->second;
    return true;
}

// item-slices per pass: the caller's cap (xsq_demixer_set_max_rows) inside what the offsets allow for J sources
static int item_cap(const xsq_demixer* d, int J) {
    const int hard = default_max_item_slices(d->plan, J);
    return d->max_item_slices > 0 ? std::min(d->max_item_slices, hard) : hard;
}

// Device tables and workspace sizes of a new plan, after room was made for it (a known shape never comes here, so a cache hit
// never evicts); the plan enters the cache once its tables are on the device.
static int publish_plan(xsq_demixer* d, const xsq_model* Mo, const std::vector<int64_t>& key, PlanBuild& pb, int wiener, ForwardPlan** out) {
    if (int rc = evict_for_new_plan(d)) return rc;
    ForwardPlan& fp = pb.fp;
    const size_t total = pb.rows.size(), J = sources_of(Mo);
    XSQ_HIP(hipMalloc(&fp.d_tables, std::max<size_t>(total, 1) * sizeof(int64_t)));
    if (hipHostMalloc(&fp.h_tables, std::max<size_t>(total, 1) * sizeof(int64_t), hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(fp.d_tables);
        set_error("xsq_separator_forward: hipHostMalloc of %zu table words failed", total);
        return XSQ_ERR_HIP;
    }
    fp.table_words = total;
    std::copy(pb.rows.begin(), pb.rows.end(), fp.h_tables);
    size_t o = 0;
    for (PassPlan& p : fp.passes) {
        p.d_xrows = fp.d_tables + o; o += (size_t)2 * p.B;
        p.d_orows = fp.d_tables + o; o += 2 * J * p.B;
        PassLayout L;
        if (int rc = pass_layout(d, Mo, p.B, p.n_pad, wiener, &L)) { (void)hipFree(fp.d_tables); (void)hipHostFree(fp.h_tables); return rc; }
        size_t& dst = p.tail ? fp.tail_bytes : fp.main_bytes;
        dst = std::max(dst, L.total);
    }
    fp.main_bytes += al256(fp.ext_floats * 4);
    fp.last_use = ++d->clock;
    // The tables are on the device before the plan is visible to any caller (any thread, any stream, eager or capturing):
    // copied on the demixer's own non-blocking stream and waited for on the host -- microseconds per NEW shape, no wait for
    // other streams' work.  A plan cannot be made while a stream of this thread is capturing in global mode (the wait is
    // refused): size the call first (xsq_separator_workspace), then capture.
    hipError_t ue = hipMemcpyAsync(fp.d_tables, fp.h_tables, fp.table_words * sizeof(int64_t), hipMemcpyHostToDevice, d->up_stream);
    if (ue == hipSuccess) ue = hipStreamSynchronize(d->up_stream);
    if (ue != hipSuccess) {
        (void)hipFree(fp.d_tables); (void)hipHostFree(fp.h_tables);
        set_error("xsq_separator_forward: upload of the row tables of a new call shape -> %s (a new shape cannot be planned during "
                  "stream capture: call xsq_separator_workspace for it first)", hipGetErrorString(ue));
        return XSQ_ERR_HIP;
    }
    auto ins = d->plans.emplace(key, fp);
    *out = &ins.first->second;
    return XSQ_OK;
}

// The schedule with its device tables and workspace sizes.
static int get_forward_plan(xsq_demixer* d, const xsq_model* Mo, int nb, int64_t N, int64_t cs, int max_stack, int wiener, ForwardPlan** out) {
    xsq_plan* P = d->plan;
    const int J = sources_of(Mo);
    const std::vector<int64_t> key{nb, N, cs, max_stack, wiener, d->max_item_slices, Mo->causal | ((int64_t)Mo->wiener_flags << 8)};
    if (cached_plan(d, key, out)) return XSQ_OK;
    const int64_t min_samples = P->L / 2 + 1;                      // separator.py:162
    PlanBuild pb;
    ForwardPlan& fp = pb.fp;
    std::vector<SchedPass> sched;
    build_schedule(P->L, nb, N, cs, max_stack, wiener ? 1 : 0, item_cap(d, J), &sched);
    for (const SchedPass& sp : sched) {
        PassPlan p;
        p.n = sp.n; p.n_pad = std::max(sp.n, min_samples); p.B = sp.k * sp.nbb; p.group = sp.nbb; p.tail = sp.tail;
        p.set_first = sp.set_first; p.set_count = sp.set_count;
        // chunk j of the pass, sample b0 + b of the batch: where the chunk lies in the (nb, 2, N) input and the (J, nb, 2, N) result
        auto at = [&](int64_t lead, int item, int c) { return ((lead + sp.b0 + item % sp.nbb) * 2 + c) * N + sp.start + item / sp.nbb * cs; };
        pb.add_pass(p, J, [&](int item, int c) { return at(0, item, c); }, [&](int t, int item, int c) { return at((int64_t)t * nb, item, c); });
    }
    // the window-maximum tables of the split sets (one per set, shared by its passes)
    for (size_t i = 0; i < sched.size(); ++i) {
        if (!sched[i].needs_ext || (int)i != sched[i].set_first) continue;
        const int64_t off = (int64_t)fp.ext_floats;
        fp.ext_floats += (size_t)xsq_wiener_num_windows(P->nblocks, d->F.data(), d->T.data(), sched[i].k,
                                                        xsq_plan_num_slices(P, fp.passes[i].n_pad), 5000, 1);
        for (int q = 0; q < sched[i].set_count; ++q) fp.passes[i + q].ext_off = off;
    }
    return publish_plan(d, Mo, key, pb, wiener, out);
}


// ---- overlapped segments (separate_sources, cadenza/enhance.py:35-99): the segment rule of include/xumx_slicq_hip.h in
// integers, pure host arithmetic (tests/test_overlap_cpu.py drives it through xsq_segment_schedule).
struct Segment { int64_t start, n; int fade_in, fade_out; };

static void build_segments(int64_t N, int64_t cl, int64_t ov, std::vector<Segment>* out) {
    auto start_of = [&](int64_t k) { return k == 0 ? (int64_t)0 : k * cl - ov; };
    for (int64_t k = 0; start_of(k) < N - ov; ++k) {
        const bool next = start_of(k + 1) < N - ov;
        out->push_back(Segment{start_of(k), std::min((k + 1) * cl, N) - start_of(k), k == 0 ? 0 : (int)ov, next ? (int)ov : 0});
    }
}

// Passes of equal-length segments one chunk_len apart (the first segment, the middle ones, the last: with ov == 0 the
// first belongs to the middle ones), each of at most `budget` item-slices; every segment carries the whole batch.
static int get_segment_plan(xsq_demixer* d, const xsq_model* Mo, int nb, int64_t N, int64_t cs, int64_t cl, int64_t ov, int max_stack,
                            int wiener, ForwardPlan** out) {
    xsq_plan* P = d->plan;
    // (nine words: never the seven of an xsq_separator_forward shape)
    const int J = sources_of(Mo);
    const std::vector<int64_t> key{nb, N, cs, max_stack, wiener, d->max_item_slices, Mo->causal | ((int64_t)Mo->wiener_flags << 8), cl, ov};
    if (cached_plan(d, key, out)) return XSQ_OK;
    const int h = P->L / 4;
    const int64_t min_samples = P->L / 2 + 1;
    const int64_t hard = default_max_item_slices(P, J);
    // what bounds a stacked pass of full chunks today: max_stack items of a full chunk's slices, and the cap
    const int64_t S_full = slices_of(std::max(cs, min_samples), h);
    const int64_t budget = std::min<int64_t>(item_cap(d, J), (max_stack > hard / S_full) ? hard : max_stack * S_full);
    std::vector<Segment> segs;
    build_segments(N, cl, ov, &segs);
    PlanBuild pb;
    for (size_t s0 = 0; s0 < segs.size();) {
        const int64_t n = segs[s0].n, n_pad = std::max(n, min_samples);
        const int64_t S = slices_of(n_pad, h);
        XSQ_REQUIRE((int64_t)nb * S <= hard, "xsq_separator_forward_segments: nb=%d samples of %lld slices exceed one pass (%lld item-slices): "
                    "split the batch", nb, (long long)S, (long long)hard);
        const int64_t per_pass = std::max<int64_t>(1, budget / ((int64_t)nb * S));
        size_t s1 = s0 + 1;
        while (s1 < segs.size() && (int64_t)(s1 - s0) < per_pass && segs[s1].n == n && segs[s1].start - segs[s1 - 1].start == cl) ++s1;
        PassPlan p;
        p.seg_k = (int)(s1 - s0); p.seg_start = segs[s0].start; p.seg_stride = cl;
        p.fade_in = segs[s0].fade_in ? 1 : 0; p.fade_out = segs[s1 - 1].fade_out ? 1 : 0;
        p.n = n; p.n_pad = n_pad; p.B = p.seg_k * nb; p.group = nb;
        // segment j of the pass, sample b: read where it lies in the input, written as (J, B, 2, n) into the scratch arena
        pb.add_pass(p, J, [&](int item, int c) { return ((int64_t)(item % nb) * 2 + c) * N + segs[s0 + item / nb].start; },
                    [&](int t, int item, int c) { return (((int64_t)t * p.B + item) * 2 + c) * n; });
        pb.fp.scratch_bytes = std::max(pb.fp.scratch_bytes, al256((size_t)2 * J * p.B * n * sizeof(float)));
        s0 = s1;
    }
    return publish_plan(d, Mo, key, pb, wiener, out);
}

static int check_call(const char* who, int nb, int64_t N, int64_t cs, int max_stack, int wiener) {
    XSQ_REQUIRE(nb > 0 && N > 0 && cs > 0 && max_stack > 0, "%s: nb=%d N=%lld chunk_size=%lld max_stack=%d", who, nb, (long long)N, (long long)cs, max_stack);
    XSQ_REQUIRE(wiener >= 0, "%s: wiener=%d iterations", who, wiener);
    return XSQ_OK;
}

static int check_segments(const char* who, int nb, int64_t N, int64_t cs, int64_t cl, int64_t ov, int max_stack, int wiener) {
    if (int rc = check_call(who, nb, N, cs, max_stack, wiener)) return rc;
    XSQ_REQUIRE(cl >= 1, "%s: chunk_len=%lld samples per segment (>= 1)", who, (long long)cl);
    XSQ_REQUIRE(ov >= 0, "%s: ov=%lld overlapping samples (>= 0)", who, (long long)ov);
    XSQ_REQUIRE(ov < cl, "%s: ov=%lld >= chunk_len=%lld: segments two apart would overlap", who, (long long)ov, (long long)cl);
    XSQ_REQUIRE(cl <= cs && ov <= cs - cl, "%s: a segment of chunk_len + ov = %lld + %lld samples is longer than chunk_size=%lld", who, (long long)cl,
                (long long)ov, (long long)cs);
    XSQ_REQUIRE(N > ov, "%s: N=%lld samples are not more than ov=%lld: no segment exists", who, (long long)N, (long long)ov);
    return XSQ_OK;
}

// The plan `get` finds or makes under the demixer's lock, for a call that launches on `stream`: while that stream is
// capturing, the plan is pinned (the graph's nodes will hold its tables).
template <class Get> static int acquire_plan(xsq_demixer* d, hipStream_t stream, Get get, ForwardPlan** fp) {
    std::lock_guard<std::mutex> lk(d->mu);
    if (int rc = get(fp)) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) (*fp)->pinned = true;
    return XSQ_OK;
}

// ---- the streaming session (Separator.stream): steps on the absolute block grid, pure host arithmetic ------------------
// Block k = samples [2kh, (2k + 2)h) = second half of slice k + first half of slice k + 1.  Step j closes the blocks
// [j m, (j + 1) m): it inverts the slices (j m, (j + 1) m] (and slice 0 in step 0) with masks from a CDAE window that reaches
// `back` slices behind the first and `ahead` beyond the last of them, clipped to the slices the signal has.
struct StreamStep { int64_t block0; int blocks; int64_t first, w0, w1, trigger; };

// total < 0: the stream is open (no last slice to clip at)
static bool stream_step(int h, int m, int back, int ahead, int64_t j, int64_t total, StreamStep* o) {
    const int64_t S = total < 0 ? (1ll << 60) : slices_of(std::max<int64_t>(total, 2 * h + 1), h);      // separator.py:162: at least L/2 + 1 samples
    const int64_t nblk = total < 0 ? (1ll << 60) : (total + 2 * h - 1) / (2 * h);
    o->block0 = j * m;
    if (o->block0 >= nblk) return false;
    o->blocks = (int)std::min<int64_t>(m, nblk - o->block0);
    o->first = j == 0 ? 0 : o->block0 + 1;
    const int64_t last = o->block0 + o->blocks;
    o->w0 = std::max<int64_t>(0, o->first - back);
    o->w1 = std::min<int64_t>(S - 1, last + ahead);
    if (o->w1 - o->w0 < 2) o->w0 = std::max<int64_t>(0, o->w1 - 2);       // the conv stack needs 3 slices
    o->trigger = (2 * ((j + 1) * m + ahead) + 2) * h;
    return true;
}

}  // namespace

struct xsq_stream {
    xsq_demixer* d = nullptr;
    int nb = 0, m = 0, back = 0, ahead = 0;
    int ring = 0;                    // samples per channel of the audio ring
    int64_t fed = 0, steps = 0;
    int cur = 0;                     // which of the two carry buffers the next step reads
    size_t ring_bytes() const { return al256((size_t)2 * nb * ring * 4); }
    size_t carry_bytes() const { return al256((size_t)8 * nb * 2 * d->plan->h * 4); }
};

namespace {

// grid (ceil(count / 256), 2 nb): sample i of row r of the block goes to ring position (fed + i) % ring
__global__ __launch_bounds__(256) void k_ring_write(const float* __restrict__ x, int64_t row_stride, float* __restrict__ ring_buf, int ring,
                                                     int64_t fed, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int r = blockIdx.y;
    ring_buf[(int64_t)r * ring + (fed + i) % ring] = x[(int64_t)r * row_stride + i];
}

struct StreamLayout { size_t X, masks, fwd, cdae, inv, total, fwd_bytes, cdae_bytes, inv_bytes; };

// workspace of one step: X arena of the window | masks arena of the window | forward ws | CDAE ws | emission ws
static int stream_layout(const xsq_stream* st, const xsq_model* Mo, int Sw, int Sn, StreamLayout* L) {
    xsq_plan* P = st->d->plan;
    const int B = st->nb;
    const size_t coefs = (size_t)Sw * P->sumFT;
    size_t o = 0;
    L->X = o;     o += al256((size_t)2 * B * coefs * 8);
    L->masks = o; o += al256((size_t)8 * B * coefs * 4);
    L->fwd_bytes = xsq_slicqt_forward_workspace(P, 2 * B, (int64_t)(2 * Sw - 3) * P->h);      // (that many samples give Sw slices)
    L->cdae_bytes = xsq_cdae_workspace(Mo, B, Sw);
    L->inv_bytes = xsq_slicqt_inverse_carry_workspace(P, 8 * B, 2 * B, Sn);
    if (!L->fwd_bytes || !L->cdae_bytes || !L->inv_bytes) {
        const std::string why = xsq_last_error();
        set_error("xsq_stream_step: nb=%d, a window of %d slices: a stage's workspace query failed (%s)", B, Sw, why.c_str());
        return XSQ_ERR_ARG;
    }
    L->fwd = o;  o += al256(L->fwd_bytes);
    L->cdae = o; o += al256(L->cdae_bytes);
    L->inv = o;  o += al256(L->inv_bytes);
    L->total = o + 256;
    return XSQ_OK;
}

static int stream_model_ok(const xsq_stream* st, const xsq_model* Mo, const char* who) {
    xsq_plan* P = st->d->plan;
    XSQ_REQUIRE(Mo->sumFT == P->sumFT && Mo->nblocks == P->nblocks, "%s: the model's block table is not the plan's", who);
    XSQ_REQUIRE(!Mo->wiener_flags, "%s: softmask / residual are options of the Wiener filter, whose statistics span a 5000-frame window: "
                "a streaming session is mix-phase", who);
    XSQ_REQUIRE(st->back >= (Mo->causal ? XSQ_STREAM_BACK_CAUSAL : XSQ_STREAM_BACK_OFFLINE), "%s: the masks of a slice depend on %d slices "
                "behind it (session: %d)", who, Mo->causal ? XSQ_STREAM_BACK_CAUSAL : XSQ_STREAM_BACK_OFFLINE, st->back);
    return XSQ_OK;
}

}  // namespace

extern "C" {

int xsq_stream_schedule(int64_t N, int L, int hop_slices, int back, int ahead, int64_t* steps, int max_steps) {
    XSQ_REQUIRE(N >= 0 && L > 0 && L % 4 == 0 && hop_slices >= 1 && back >= 0 && ahead >= 0 && (steps || max_steps <= 0),
                "xsq_stream_schedule: N=%lld L=%d hop_slices=%d back=%d ahead=%d", (long long)N, L, hop_slices, back, ahead);
    XSQ_REQUIRE(N / (L / 2) / hop_slices < (1 << 30), "xsq_stream_schedule: N=%lld in steps of %d blocks", (long long)N, hop_slices);
    StreamStep sp;
    int64_t j = 0;
    for (; stream_step(L / 4, hop_slices, back, ahead, j, N, &sp); ++j)
        if (j < max_steps) {
            int64_t* o = steps + 6 * j;
            o[0] = sp.block0; o[1] = sp.blocks; o[2] = sp.first; o[3] = sp.w0; o[4] = sp.w1; o[5] = sp.trigger;
        }
    return (int)j;
}

int xsq_stream_create(xsq_stream** out, xsq_demixer* d, const xsq_model* Mo, int nb, int hop_slices, int back, int ahead) {
    XSQ_REQUIRE(out && d && Mo, "xsq_stream_create: null argument");
    XSQ_REQUIRE(nb >= 1 && hop_slices >= 1 && hop_slices <= 4096, "xsq_stream_create: nb=%d hop_slices=%d", nb, hop_slices);
    XSQ_REQUIRE(ahead >= XSQ_STREAM_AHEAD && back <= 64 && ahead <= 64, "xsq_stream_create: back=%d ahead=%d (the masks of a slice depend on %d "
                "slices beyond it)", back, ahead, XSQ_STREAM_AHEAD);
    xsq_stream* st = new xsq_stream();
    st->d = d; st->nb = nb; st->m = hop_slices; st->back = back; st->ahead = ahead;
    // from the first sample of the oldest window slice, (2 (j m + 1 - back) - 2) h, to the trigger of the step, (2 ((j + 1) m + ahead) + 2) h
    st->ring = (2 * (back + ahead + hop_slices) + 2) * d->plan->h;
    if (int rc = stream_model_ok(st, Mo, "xsq_stream_create")) { delete st; return rc; }
    *out = st;
    return XSQ_OK;
}

int xsq_stream_destroy(xsq_stream* st) { delete st; return XSQ_OK; }

size_t xsq_stream_state_bytes(const xsq_stream* st) { return st ? st->ring_bytes() + 2 * st->carry_bytes() : 0; }

size_t xsq_stream_workspace(const xsq_stream* st, const xsq_model* Mo) {
    if (!st || !Mo || stream_model_ok(st, Mo, "xsq_stream_workspace")) return 0;
    size_t need = 0;
    for (int Sw = 3; Sw <= st->m + st->back + st->ahead + 1; ++Sw) {
        StreamLayout L;
        if (stream_layout(st, Mo, Sw, std::min(Sw, st->m + 1), &L)) return 0;
        need = std::max(need, L.total);
    }
    return need;
}

int64_t xsq_stream_next_trigger(const xsq_stream* st) {
    if (!st) return XSQ_ERR_ARG;
    StreamStep sp;
    stream_step(st->d->plan->h, st->m, st->back, st->ahead, st->steps, -1, &sp);
    return sp.trigger;
}

int xsq_stream_push(xsq_stream* st, void* state, const float* x, int64_t row_stride, int64_t count, void* stream) {
    XSQ_REQUIRE(st && state && x, "xsq_stream_push: null argument");
    XSQ_REQUIRE(count >= 1 && row_stride >= count, "xsq_stream_push: %lld samples per row, row stride %lld", (long long)count, (long long)row_stride);
    // the ring holds what the next step's window needs as long as nothing is written past that step's trigger
    XSQ_REQUIRE(st->fed + count <= xsq_stream_next_trigger(st), "xsq_stream_push: %lld + %lld samples pass the trigger of step %lld (%lld): run "
                "xsq_stream_step first", (long long)st->fed, (long long)count, (long long)st->steps, (long long)xsq_stream_next_trigger(st));
    hipLaunchKernelGGL(k_ring_write, dim3((unsigned)((count + 255) / 256), 2 * st->nb), dim3(256), 0, (hipStream_t)stream, x, row_stride,
                       (float*)state, st->ring, st->fed, (int)count);
    XSQ_HIP(hipGetLastError());
    st->fed += count;
    return XSQ_OK;
}

int xsq_stream_step(xsq_stream* st, xsq_model* Mo, void* state, const float* x, int64_t row_stride, int64_t count, int64_t total, float* out,
                    int64_t out_stride, int64_t length, void* ws, size_t ws_bytes, void* stream) {
    XSQ_REQUIRE(st && Mo && state && out && ws, "xsq_stream_step: null argument");
    if (int rc = stream_model_ok(st, Mo, "xsq_stream_step")) return rc;
    XSQ_REQUIRE(count >= 0 && (count == 0 || (x && row_stride >= count)), "xsq_stream_step: %lld new samples per row, row stride %lld",
                (long long)count, (long long)row_stride);
    // the samples that release the step ride on its first kernel, which stores them to the ring (xsq_slicqt_forward_ring)
    XSQ_REQUIRE(count == 0 || (total < 0 && st->fed + count == xsq_stream_next_trigger(st)), "xsq_stream_step: %lld + %lld samples are not the %lld "
                "that release step %lld", (long long)st->fed, (long long)count, (long long)xsq_stream_next_trigger(st), (long long)st->steps);
    XSQ_REQUIRE(total < 0 || total == st->fed, "xsq_stream_step: the final length %lld is not the %lld samples fed", (long long)total, (long long)st->fed);
    xsq_plan* P = st->d->plan;
    const int h = P->h, B = st->nb;
    StreamStep sp;
    XSQ_REQUIRE(stream_step(h, st->m, st->back, st->ahead, st->steps, total, &sp), "xsq_stream_step: step %lld lies behind the last block of %lld "
                "samples", (long long)st->steps, (long long)total);
    XSQ_REQUIRE(total >= 0 || st->fed + count >= sp.trigger, "xsq_stream_step: step %lld needs %lld samples (%lld fed)", (long long)st->steps,
                (long long)sp.trigger, (long long)st->fed);
    const int64_t want = total < 0 ? (int64_t)sp.blocks * 2 * h : std::min<int64_t>((int64_t)sp.blocks * 2 * h, total - sp.block0 * 2 * h);
    XSQ_REQUIRE(length == want && out_stride >= length, "xsq_stream_step: step %lld emits %lld samples (length %lld, row stride %lld)",
                (long long)st->steps, (long long)want, (long long)length, (long long)out_stride);
    const int Sw = (int)(sp.w1 - sp.w0 + 1), shift = st->steps == 0 ? 0 : 1;
    const int Sn = (int)(sp.block0 + sp.blocks - sp.first + 1);
    StreamLayout L;
    if (int rc = stream_layout(st, Mo, Sw, Sn, &L)) return rc;
    XSQ_REQUIRE(L.total <= ws_bytes, "xsq_stream_step: workspace too small (%zu needed, %zu given)", L.total, ws_bytes);
    char* w = (char*)ws;
    float* X = (float*)(w + L.X);
    float* masks = (float*)(w + L.masks);
    float* ring_buf = (float*)state;
    float* carry[2] = {(float*)((char*)state + st->ring_bytes()), (float*)((char*)state + st->ring_bytes() + st->carry_bytes())};
    const float *mean, *scale;
    int split, rc;
    if ((rc = xsq_model_whitening(Mo, &mean, &scale, &split))) return rc;
    float* xin = (float*)(w + L.cdae);           // (the head of the CDAE workspace, as in a pass)
    // the forward transform of the whole window, context slices included, is recomputed every step
    if ((rc = xsq_slicqt_forward_ring(P, ring_buf, st->ring, 2 * B, sp.w0, Sw, st->fed + count, x, row_stride, count, X, xin, mean, scale, split,
                                      w + L.fwd, L.fwd_bytes, stream)))
        return rc;
    st->fed += count;
    if ((rc = xsq_cdae_forward_xin(Mo, X, B, Sw, nullptr, masks, w + L.cdae, L.cdae_bytes, stream, 1))) return rc;
    if ((rc = xsq_slicqt_inverse_masked_carry(P, masks, X, 8 * B, 2 * B, Sw, (int)(sp.first - sp.w0), Sn, shift, length, out, out_stride,
                                              carry[st->cur], carry[1 - st->cur], w + L.inv, L.inv_bytes, stream)))
        return rc;
    st->cur = 1 - st->cur;
    st->steps += 1;
    return XSQ_OK;
}

int xsq_demixer_create(xsq_demixer** out, xsq_plan* plan) {
    XSQ_REQUIRE(out && plan, "xsq_demixer_create: null argument");
    xsq_demixer* d = new xsq_demixer();
    d->plan = plan;
    for (const BlockHost& b : plan->blocks) { d->F.push_back(b.F); d->T.push_back(b.T); }
    hipError_t e = hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->up_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error("xsq_demixer_create: hipEventCreate -> %s", hipGetErrorString(e));
        delete d;
        return XSQ_ERR_HIP;
    }
    *out = d;
    return XSQ_OK;
}

int xsq_demixer_destroy(xsq_demixer* d) {
    if (!d) return XSQ_OK;
    for (auto& kv : d->plans) { (void)hipFree(kv.second.d_tables); (void)hipHostFree(kv.second.h_tables); }
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    if (d->ev_join) (void)hipEventDestroy(d->ev_join);
    if (d->up_stream) (void)hipStreamDestroy(d->up_stream);
    delete d;
    return XSQ_OK;
}

int xsq_separator_schedule(int L, int64_t coefs_per_slice, int nb, int64_t N, int64_t cs, int max_stack, int wiener,
                           int max_item_slices, int64_t* passes, int max_passes) {
    XSQ_REQUIRE(L > 0 && L % 4 == 0 && coefs_per_slice > 0 && nb > 0 && N > 0 && cs > 0 && max_stack > 0 && (passes || max_passes == 0),
                "xsq_separator_schedule: bad argument");
    XSQ_REQUIRE(wiener >= 0, "xsq_separator_schedule: wiener=%d iterations", wiener);
    const int dflt = default_max_item_slices(coefs_per_slice, L / 2 + 1);      // (four sources: the schedule has no model)
    const int cap = max_item_slices > 0 ? std::min(max_item_slices, dflt) : dflt;
    std::vector<SchedPass> sched;
    build_schedule(L, nb, N, cs, max_stack, wiener ? 1 : 0, cap, &sched);
    for (size_t i = 0; i < sched.size() && (int)i < max_passes; ++i) {
        const SchedPass& p = sched[i];
        int64_t* o = passes + 8 * i;
        o[0] = p.start; o[1] = p.n; o[2] = p.k; o[3] = p.b0; o[4] = p.nbb; o[5] = p.tail; o[6] = p.set_first; o[7] = p.needs_ext;
    }
    return (int)sched.size();
}

int xsq_demixer_set_max_rows(xsq_demixer* d, int max_item_slices) {
    XSQ_REQUIRE(d, "xsq_demixer_set_max_rows: null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    d->max_item_slices = max_item_slices > 0 ? std::min(max_item_slices, default_max_item_slices(d->plan)) : 0;
    return XSQ_OK;
}

size_t xsq_demix_pass_workspace(xsq_demixer* d, const xsq_model* Mo, int B, int64_t n_pad, int wiener) {
    if (!d || !Mo || B <= 0 || n_pad <= 0 || wiener < 0) return 0;
    PassLayout L;
    return pass_layout(d, Mo, B, n_pad, wiener, &L) ? 0 : L.total;
}

int xsq_demix_pass(xsq_demixer* d, xsq_model* Mo, const float* x, const int64_t* x_rows, int B, int64_t n, int64_t n_pad,
                   int group, int wiener, float* out, const int64_t* out_rows, void* ws, size_t ws_bytes, void* stream) {
    XSQ_REQUIRE(d && Mo && x && out && out_rows && ws, "xsq_demix_pass: null argument");
    XSQ_REQUIRE(B > 0 && n > 0 && n_pad >= n, "xsq_demix_pass: B=%d n=%lld n_pad=%lld", B, (long long)n, (long long)n_pad);
    if (group <= 0) group = B;
    XSQ_REQUIRE(B % group == 0, "xsq_demix_pass: group=%d does not divide B=%d", group, B);
    XSQ_REQUIRE(wiener >= 0, "xsq_demix_pass: wiener=%d iterations", wiener);
    XSQ_REQUIRE(!(Mo->wiener_flags & XSQ_WIENER_RESIDUAL), "xsq_demix_pass: out_rows name four stems per item; the residual option "
                "(xsq_model_set_wiener_options) writes five: use xsq_separator_forward");
    PassPlan p;
    p.n = n; p.n_pad = n_pad; p.B = B; p.group = group; p.d_xrows = x_rows; p.d_orows = out_rows;
    return run_pass(d, Mo, PassInput{x, nullptr}, p, wiener, out, ws, ws_bytes, (hipStream_t)stream);
}

int xsq_separator_workspace(xsq_demixer* d, const xsq_model* Mo, int nb, int64_t N, int64_t cs, int max_stack, int wiener,
                            size_t* main_bytes, size_t* tail_bytes) {
    XSQ_REQUIRE(d && Mo && main_bytes && tail_bytes, "xsq_separator_workspace: null argument");
    if (int rc = check_call("xsq_separator_workspace", nb, N, cs, max_stack, wiener)) return rc;
    std::lock_guard<std::mutex> lk(d->mu);
    ForwardPlan* fp;
    if (int rc = get_forward_plan(d, Mo, nb, N, cs, max_stack, wiener, &fp)) return rc;
    *main_bytes = fp->main_bytes;
    *tail_bytes = fp->tail_bytes;
    return XSQ_OK;
}

static int separator_forward_impl(xsq_demixer* d, xsq_model* Mo, const float* audio, const float* const* x_slot, int nb, int64_t N, int64_t cs,
                                  int max_stack, int wiener, int overlap_tail, float* out, void* ws, size_t ws_bytes, void* tail_ws,
                                  size_t tail_ws_bytes, void* stream_, void* tail_stream_, const float* gains = nullptr, int R = 0) {
    XSQ_REQUIRE(d && Mo && (audio || x_slot) && out && ws, "xsq_separator_forward: null argument");
    if (int rc = check_call("xsq_separator_forward", nb, N, cs, max_stack, wiener)) return rc;
    hipStream_t main = (hipStream_t)stream_, side = (hipStream_t)tail_stream_;
    const PassInput in{audio, x_slot};
    ForwardPlan* fp;
    if (int rc = acquire_plan(d, main, [&](ForwardPlan** o) { return get_forward_plan(d, Mo, nb, N, cs, max_stack, wiener, o); }, &fp)) return rc;
    bool any_tail = false;
    for (const PassPlan& p : fp->passes) any_tail = any_tail || p.tail;
    const bool beside = any_tail && overlap_tail && side != main && tail_ws != nullptr;
    XSQ_REQUIRE(ws_bytes >= fp->main_bytes && (!beside || tail_ws_bytes >= fp->tail_bytes),
                "xsq_separator_forward: workspace too small (%zu / %zu needed, %zu / %zu given)", fp->main_bytes, fp->tail_bytes,
                ws_bytes, tail_ws_bytes);
    XSQ_REQUIRE(beside || ws_bytes >= std::max(fp->main_bytes, fp->tail_bytes), "xsq_separator_forward: workspace too small for the tail pass");
    int rc = XSQ_OK;
    bool forked = false;
    // The short tail chunks are launch-bound passes, independent of the stacked ones: they go out first, on the side
    // stream with their own workspace, and fill in beside the big launches; the caller's stream joins at the end -- on the
    // error paths too: whatever the side stream was given stays ordered in front of the caller's next use of `out`.
    auto join = [&]() -> int {
        if (!forked) return XSQ_OK;
        forked = false;
        XSQ_HIP(hipEventRecord(d->ev_join, side));
        XSQ_HIP(hipStreamWaitEvent(main, d->ev_join, 0));
        return XSQ_OK;
    };
    auto fail = [&](int code) { const std::string why = xsq_last_error(); (void)join(); set_error("%s", why.c_str()); return code; };
    if (beside) {
        XSQ_HIP(hipEventRecord(d->ev_fork, main));
        XSQ_HIP(hipStreamWaitEvent(side, d->ev_fork, 0));
        forked = true;
        for (const PassPlan& p : fp->passes)
            if (p.tail && (rc = run_pass(d, Mo, in, p, wiener, out, tail_ws, tail_ws_bytes, side, nullptr, gains, R))) break;
        if (rc) return fail(rc);
    }
    float* ext = (float*)ws;                                  // window-maximum tables of split sets (head of the workspace)
    const size_t ext_bytes = al256(fp->ext_floats * 4);
    char* pws = (char*)ws + ext_bytes;
    const size_t pws_bytes = ws_bytes - ext_bytes;
    if (fp->ext_floats && hipMemsetAsync(ext, 0, fp->ext_floats * 4, main) != hipSuccess) {
        (void)join();
        set_error("xsq_separator_forward: hipMemsetAsync failed");
        return XSQ_ERR_HIP;
    }
    for (size_t i = 0; i < fp->passes.size() && rc == XSQ_OK; ++i) {
        const PassPlan& p = fp->passes[i];
        if (p.tail && beside) continue;
        if (p.ext_off >= 0 && (int)i == p.set_first)       // first pass of a split set: every pass's maxima first
            for (int j = 0; j < p.set_count && rc == XSQ_OK; ++j)
                rc = run_prepass(d, Mo, in, fp->passes[i + j], pws, pws_bytes, ext, main);
        if (rc == XSQ_OK) rc = run_pass(d, Mo, in, p, wiener, out, pws, pws_bytes, main, p.ext_off >= 0 ? ext + p.ext_off : nullptr, gains, R);
    }
    return rc ? fail(rc) : join();
}

int xsq_separator_forward(xsq_demixer* d, xsq_model* Mo, const float* audio, int nb, int64_t N, int64_t cs, int max_stack,
                          int wiener, int overlap_tail, float* out, void* ws, size_t ws_bytes, void* tail_ws,
                          size_t tail_ws_bytes, void* stream_, void* tail_stream_) {
    XSQ_REQUIRE(audio, "xsq_separator_forward: null argument");
    return separator_forward_impl(d, Mo, audio, nullptr, nb, N, cs, max_stack, wiener, overlap_tail, out, ws, ws_bytes, tail_ws, tail_ws_bytes,
                                  stream_, tail_stream_);
}

int xsq_separator_forward_indirect(xsq_demixer* d, xsq_model* Mo, const float* const* audio_slot, int nb, int64_t N, int64_t cs,
                                   int max_stack, int wiener, int overlap_tail, float* out, void* ws, size_t ws_bytes, void* tail_ws,
                                   size_t tail_ws_bytes, void* stream_, void* tail_stream_) {
    XSQ_REQUIRE(audio_slot, "xsq_separator_forward_indirect: null argument");
    return separator_forward_impl(d, Mo, nullptr, audio_slot, nb, N, cs, max_stack, wiener, overlap_tail, out, ws, ws_bytes, tail_ws,
                                  tail_ws_bytes, stream_, tail_stream_);
}

int xsq_segment_schedule(int64_t N, int64_t chunk_len, int64_t ov, int64_t* segs, int max_segs) {
    XSQ_REQUIRE(N >= 1 && chunk_len >= 1 && ov >= 0 && (segs || max_segs <= 0), "xsq_segment_schedule: N=%lld chunk_len=%lld ov=%lld", (long long)N,
                (long long)chunk_len, (long long)ov);
    XSQ_REQUIRE(N / chunk_len < (1 << 30), "xsq_segment_schedule: N=%lld in segments of %lld", (long long)N, (long long)chunk_len);
    std::vector<Segment> sg;
    build_segments(N, chunk_len, ov, &sg);
    for (size_t i = 0; i < sg.size() && (int64_t)i < max_segs; ++i) {
        int64_t* o = segs + 4 * i;
        o[0] = sg[i].start; o[1] = sg[i].n; o[2] = sg[i].fade_in; o[3] = sg[i].fade_out;
    }
    return (int)sg.size();
}

int xsq_separator_segments_workspace(xsq_demixer* d, const xsq_model* Mo, int nb, int64_t N, int64_t cs, int64_t cl, int64_t ov, int max_stack,
                                     int wiener, size_t* bytes) {
    XSQ_REQUIRE(d && Mo && bytes, "xsq_separator_segments_workspace: null argument");
    if (int rc = check_segments("xsq_separator_segments_workspace", nb, N, cs, cl, ov, max_stack, wiener)) return rc;
    std::lock_guard<std::mutex> lk(d->mu);
    ForwardPlan* fp;
    if (int rc = get_segment_plan(d, Mo, nb, N, cs, cl, ov, max_stack, wiener, &fp)) return rc;
    *bytes = fp->scratch_bytes + fp->main_bytes;
    return XSQ_OK;
}

int xsq_separator_forward_segments(xsq_demixer* d, xsq_model* Mo, const float* audio, int nb, int64_t N, int64_t cs, int64_t cl, int64_t ov,
                                   int max_stack, int wiener, float* out, void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(d && Mo && audio && out && ws, "xsq_separator_forward_segments: null argument");
    if (int rc = check_segments("xsq_separator_forward_segments", nb, N, cs, cl, ov, max_stack, wiener)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    ForwardPlan* fp;
    if (int rc = acquire_plan(d, stream, [&](ForwardPlan** o) { return get_segment_plan(d, Mo, nb, N, cs, cl, ov, max_stack, wiener, o); }, &fp))
        return rc;
    XSQ_REQUIRE(ws_bytes >= fp->scratch_bytes + fp->main_bytes, "xsq_separator_forward_segments: workspace too small (%zu needed, %zu given)",
                fp->scratch_bytes + fp->main_bytes, ws_bytes);
    // scratch (the un-faded stems of one pass) | workspace of the pass.  In segment order on ONE stream: the head of a
    // pass's first segment is added onto what the launch of the previous pass stored.
    float* scratch = (float*)ws;
    char* pws = (char*)ws + fp->scratch_bytes;
    for (const PassPlan& p : fp->passes) {
        if (int rc = run_pass(d, Mo, PassInput{audio, nullptr}, p, wiener, scratch, pws, ws_bytes - fp->scratch_bytes, stream)) return rc;
        if (int rc = xsq_crossfade_place_sources(scratch, p.d_orows, out, sources_of(Mo), nb, N, p.seg_start, p.seg_stride, p.n, p.seg_k, (int)ov,
                                                 p.fade_in, p.fade_out, stream))
            return rc;
    }
    return XSQ_OK;
}

// ---- the ideal-mask oracle (slicqfinder.py:43-117): forward of the stems -> filter in place -> inverse ------------------
namespace {

struct IdealLayout { size_t Y, tf, wien, total, Y_bytes, tf_bytes, wien_bytes; int S; };

// workspace of a call: the arena of the 8B channels | transform ws (forward, then inverse: one after the other) | statistics.
// XSQ_ERR_ARG, with the reason, for a shape the stages would refuse: nothing is launched for it.
static int ideal_layout(const char* who, xsq_demixer* d, int B, int64_t n, int strategy, int win_len, IdealLayout* L) {
    XSQ_REQUIRE(d, "%s: null demixer", who);
    XSQ_REQUIRE(B > 0 && n > 0, "%s: B=%d n=%lld", who, B, (long long)n);
    XSQ_REQUIRE(strategy == XSQ_IDEAL_WIENER || strategy == XSQ_IDEAL_PHASEMIX, "%s: strategy=%d (XSQ_IDEAL_WIENER, XSQ_IDEAL_PHASEMIX)", who,
                strategy);
    XSQ_REQUIRE(win_len >= 0, "%s: win_len=%d (0: one window over all frames)", who, win_len);
    xsq_plan* P = d->plan;
    const int S = xsq_plan_num_slices(P, n);
    XSQ_REQUIRE(S >= 2, "%s: %lld samples give %d slices", who, (long long)n, S);
    XSQ_REQUIRE((int64_t)B * S <= default_max_item_slices(P), "%s: B=%d items of %d slices exceed one launch (%d item-slices): fewer items or "
                "shorter pieces", who, B, S, default_max_item_slices(P));
    int64_t rows = 0;
    for (int32_t f : d->F) rows += (int64_t)B * f;
    XSQ_REQUIRE(rows <= 65535, "%s: %lld (item, bin) rows exceed one launch", who, (long long)rows);
    L->S = S;
    L->Y_bytes = (size_t)8 * B * S * P->sumFT * 8;
    L->tf_bytes = std::max(xsq_slicqt_forward_workspace(P, 8 * B, n), xsq_slicqt_inverse_workspace(P, 8 * B, S));
    L->wien_bytes = strategy == XSQ_IDEAL_WIENER ? xsq_wiener_sources_workspace(P->nblocks, d->F.data(), d->T.data(), B, S, win_len) : 0;
    if (!L->tf_bytes || (strategy == XSQ_IDEAL_WIENER && !L->wien_bytes)) {
        const std::string why = xsq_last_error();
        set_error("%s: B=%d, %lld samples: a stage's workspace query failed (%s)", who, B, (long long)n, why.c_str());
        return XSQ_ERR_ARG;
    }
    size_t o = 0;
    L->Y = o;    o += al256(L->Y_bytes);
    L->tf = o;   o += al256(L->tf_bytes);
    L->wien = o; o += al256(L->wien_bytes);
    L->total = o + 256;
    return XSQ_OK;
}

}  // namespace

size_t xsq_ideal_workspace(xsq_demixer* d, int B, int64_t n, int strategy, int win_len) {
    IdealLayout L;
    return ideal_layout("xsq_ideal_workspace", d, B, n, strategy, win_len, &L) ? 0 : L.total;
}

int xsq_ideal_separate(xsq_demixer* d, const float* sources, int B, int64_t n, int strategy, int win_len, float* estimates, void* ws,
                       size_t ws_bytes, void* stream) {
    XSQ_REQUIRE(d && sources && estimates && ws, "xsq_ideal_separate: null argument");
    IdealLayout L;
    if (int rc = ideal_layout("xsq_ideal_separate", d, B, n, strategy, win_len, &L)) return rc;
    if (L.total > ws_bytes) {
        set_error("xsq_ideal_separate: workspace too small (%zu needed, %zu given)", L.total, ws_bytes);
        return XSQ_ERR_WORKSPACE;
    }
    xsq_plan* P = d->plan;
    char* w = (char*)ws;
    float* Y = (float*)(w + L.Y);
    if (int rc = xsq_slicqt_forward(P, sources, 8 * B, n, Y, w + L.tf, L.tf_bytes, stream)) return rc;
    if (strategy == XSQ_IDEAL_WIENER) {
        if (int rc = xsq_wiener_em_sources(P->nblocks, d->F.data(), d->T.data(), Y, Y, B, L.S, win_len, 1, w + L.wien, L.wien_bytes, stream))
            return rc;
    } else if (int rc = xsq_phasemix_sources(P->nblocks, d->F.data(), d->T.data(), Y, Y, B, L.S, stream)) {
        return rc;
    }
    return xsq_slicqt_inverse(P, Y, 8 * B, L.S, n, estimates, w + L.tf, L.tf_bytes, stream);
}

int xsq_separator_remix(xsq_demixer* d, xsq_model* Mo, const float* audio, int nb, int64_t N, int64_t cs, int max_stack, int wiener,
                        int overlap_tail, float* out, void* ws, size_t ws_bytes, void* tail_ws, size_t tail_ws_bytes, void* stream_,
                        void* tail_stream_, const float* gains, int R) {
    XSQ_REQUIRE(audio && gains, "xsq_separator_remix: null argument");
    XSQ_REQUIRE(R >= 1 && R <= 4, "xsq_separator_remix: R=%d mixes (1..4)", R);
    for (int i = 0; i < 4 * R; ++i) XSQ_REQUIRE(std::isfinite(gains[i]), "xsq_separator_remix: gain [%d][%d] is not finite", i / 4, i % 4);
    XSQ_REQUIRE(Mo && !(Mo->wiener_flags & XSQ_WIENER_RESIDUAL), "xsq_separator_remix: the residual option has no gain column; remix the "
                "four targets without it");
    return separator_forward_impl(d, Mo, audio, nullptr, nb, N, cs, max_stack, wiener, overlap_tail, out, ws, ws_bytes, tail_ws, tail_ws_bytes,
                                  stream_, tail_stream_, gains, R);
}

}  // extern "C"
