// api_index.hip — C-ABI of the flat cosine index (the chromadb Collection's numeric half) and the two
// stateless glue kernels (blend, shard merge).
#include "common.h"
#include <queue>
#include "retrieval_kernels.h"
#include "membership_kernels.h"
#include "assign_kernels.h"
#include "partition_kernels.h"
#include "distinct_kernels.h"
#include "subset_kernels.h"
#include "after_kernels.h"
#include "grouped_kernels.h"
#include "gemm_bf16_256.h"
#include "gemm_strip_p256.h"
#include <algorithm>
#include "index_plans.h"

static_assert(PLAN_SELECT_UNIT == SELECT_UNIT && PLAN_PROBE_SEG == PROBE_SEG, "index_plans.h repeats what the kernel headers fix");
static_assert(PLAN_DISTINCT_THREADS == DISTINCT_THREADS && PLAN_DISTINCT_SLOTS == DISTINCT_SLOTS && PLAN_DISTINCT_MAX_POOL < DISTINCT_SLOTS,
              "index_plans.h repeats what distinct_kernels.h fixes");
static_assert(PLAN_SUBSET_BLOCK_ROWS == SUBSET_BLOCK_ROWS, "index_plans.h repeats what subset_kernels.h fixes");
static_assert(PLAN_GROUPED_THREADS == GROUPED_THREADS && PLAN_GROUPED_SLOTS == GROUPED_SLOTS && PLAN_GROUPED_MAX_POOL < GROUPED_SLOTS &&
                  PLAN_GROUPED_WALK_LDS == GROUPED_WALK_LDS && PLAN_GROUPED_MAX_GROUPS == MMISS_MAX_GROUPS,
              "index_plans.h repeats what grouped_kernels.h and mmiss.h fix");

// The results of a query-like call of Q queries: `slots` labels and distances and a count per query, for some calls a total and
// a flag per query. lab / tot / dist / cnt are where the kernels write them: the caller's device buffers, or a pinned host block
// the last kernel writes straight into — the call then ends with ONE stream synchronisation and no copy-engine operation (round
// 3: four small device-to-host copies used to sit there, ~25 us) — and deliver() hands over. Flags are the host's own and always
// lie in the pinned block. The block's layout and grow rule: result_layout (index_plans.h).
struct ResultBlock {
    int64_t* lab = nullptr; int64_t* tot = nullptr; float* dist = nullptr; int32_t* cnt = nullptr; int32_t* flags = nullptr;
    bool dev = false;
    int64_t Q = 0, slots = 0;
    int64_t* out_lab = nullptr; int64_t* out_tot = nullptr; float* out_dist = nullptr; int32_t* out_cnt = nullptr;   // the caller's
    // out_cnt_ / out_tot_ may be null: device outputs then leave cnt / tot null for the caller to point at scratch of its own
    int stage(PinBuf& pin, hipStream_t st, int64_t Q_, int64_t slots_, bool dev_, bool totals, bool with_flags, int64_t* out_lab_,
              float* out_dist_, int32_t* out_cnt_, int64_t* out_tot_) {
        Q = Q_; slots = slots_; dev = dev_;
        lab = out_lab = out_lab_; dist = out_dist = out_dist_; cnt = out_cnt = out_cnt_; tot = out_tot = out_tot_;
        flags = nullptr;
        if (dev && !with_flags) return MMISS_OK;
        const ResultLayout l = result_layout(Q, slots, totals, with_flags);
        MM_TRY(pin.ensure(l.need, st, l.grow));
        char* const b = pin.as<char>();
        if (with_flags) flags = reinterpret_cast<int32_t*>(b + l.flags);
        if (!dev) {
            lab = reinterpret_cast<int64_t*>(b); tot = totals ? reinterpret_cast<int64_t*>(b + l.tot) : nullptr;
            dist = reinterpret_cast<float*>(b + l.dist); cnt = reinterpret_cast<int32_t*>(b + l.cnt);
        }
        return MMISS_OK;
    }
    // host outputs, once the stream has drained
    void deliver() const {
        if (dev) return;
        memcpy(out_lab, lab, (size_t)Q * slots * 8);
        memcpy(out_dist, dist, (size_t)Q * slots * 4);
        if (out_cnt) memcpy(out_cnt, cnt, (size_t)Q * 4);
        if (out_tot) memcpy(out_tot, tot, (size_t)Q * 8);
    }
};

struct mmiss_index {
    int dim = 0, dtype = MMISS_F32, device = 0, elt = 4;
    int qelt() const { return dtype == MMISS_F32 ? 4 : 2; }   // bytes per element of the scan's query operand (f16 for f16 and fp8 rows)
    hipStream_t own_stream = nullptr, user_stream = nullptr;
    bool has_user_stream = false;
    // a call that returns with work still queued on a caller's stream (device outputs) marks its end with this event;
    // switching streams waits for exactly that work, not for whatever else the caller has put on the stream since
    hipEvent_t done_ev = nullptr;
    bool async_pending = false;
    // The handle's second stream: every widen pass runs here, beside whatever the caller has queued on stream() since
    // mmiss_index_query_begin (see query_end_locked). No event ties it to stream() in either direction: the host has seen the
    // first pass finish before it queues anything here, and drains it before query_end returns.
    hipStream_t side_stream = nullptr;
    std::mutex mu;
    int64_t count = 0, capacity = 0;
    DevBuf rows, labels_d;
    DevBuf inv;   // MMISS_F8 only: [capacity] f32, inverse norm of every row's values (f8_row_inv_kernel); zero behind count
    std::vector<int64_t> labels_h;
    // per-row 64-bit tag words of filtered queries (mmiss_index_set_tags): [capacity] u64 on the device, zero behind count, and
    // their host mirror beside labels_h (the exhaustive pass selects on the host)
    DevBuf tags;
    std::vector<uint64_t> tags_h;
    // a filtered query's masks on the device (Pending::d_mask points here); fmask2 holds the masks of the flagged queries in the
    // widen pass's compacted order
    DevBuf fmask, fmask2, tag_stage;
    // scratch
    DevBuf stage, qn, qs, qstage, lists_s, lists_r, lists2_s, lists2_r, cand, cur_s, cur_r, out_c, map, gmax;
    // exactness guard + widen pass (see "exactness contract" above mmiss_index_query)
    DevBuf qmap, qmap64, qs2, cand2;
    DevBuf eps_q, thr, thr2, swp_cnt, swp_list;   // per-query error bound, sweep thresholds (all / flagged queries), appended rows
    DevBuf seed_s, seed_r, fcnt, fbuf_s, fbuf_g;  // threshold-filtered selection (Q > 128)
    PinBuf pin;       // the pinned block of a call's ResultBlock: the guard's per-query flags always, host outputs on their way out
    PinBuf swp_pin;   // the widen pass's list lengths, written by the re-rank kernel itself (RerankArgs::cnt_host)
    int64_t stat_queries = 0, stat_flagged = 0, stat_rounds = 0, stat_pages = 0, stat_exhaustive = 0, stat_swept_rows = 0;
    // a query between mmiss_index_query_begin and mmiss_index_query_end: its first pass is queued, `done_ev` marks its end
    struct Pending {
        bool active = false, guard = false;
        int Q = 0, k = 0;
        ResultBlock out;   // k slots per query, and the guard's flags
        // the predicate of a filtered query (mmiss_index_query_filtered*; filt = false for an unfiltered one): [Q] required and
        // [Q] excluded masks on the host (the widen pass's compaction and the exhaustive pass read them) and on the device
        bool filt = false;
        std::vector<uint64_t> req, exc;
        const uint64_t* d_mask = nullptr;   // [Q] required, then [Q] excluded
    } pend;
    DevBuf dist_all;  // exhaustive fallback: one canonical distance per row
    PinBuf dist_pin;  // ... and the pinned host block they come back through
    // radius queries (mmiss_index_query_radius*): a chunk's radii, its queries' own rows (later_only) and, when the caller
    // passes no out_total, the totals; the queries served and the passes over the index they cost
    DevBuf rad, row_min, rtotal;
    int64_t stat_radius_queries = 0, stat_radius_pages = 0;
    // membership / tagging (mmiss_index_membership, mmiss_index_tag_by_radius): the words when the caller's are host memory or
    // the call merges them into the tags; radii, the two thresholds per probe and the tag form's bits ([64] each); the counts
    DevBuf mem_words, mem_thr, mem_cnt;
    // assignment / clustering (mmiss_index_assign, mmiss_index_cluster_sums): the scan's per-row state (s1, i1, s2: [count] each),
    // the borderline rows, the assignment and distances when the caller's are host memory (and a host assignment of
    // cluster_sums), the sums when the caller's are host memory, and the small block: E, live centres, borderline rows, sizes
    DevBuf asg_state, asg_list, asg_out, asg_sums, asg_meta;
    // partitioned search (mmiss_index_partition_set, mmiss_index_query_probed): the partition — C = 0: none — with the normalised
    // centres, the cell of each of the first B rows, the rows grouped by cell, the cell offsets, the host mirror of the sizes and
    // top_prefix[j] = the sum of the j largest of them (the bound on a query's candidates); the queries served and rows scanned
    // since it was set. Dropped by whatever moves or changes rows (drop_partition).
    struct Partition {
        int C = 0;
        int64_t B = 0, in_cells = 0, largest = 0, empty = 0;
        DevBuf cn, cells, order, off;
        std::vector<int64_t> sizes, top_prefix;
        int64_t queries = 0, scanned = 0;
    } part;
    // ... and a probed call's scratch: the probed cells, their key offsets and the totals per query of a chunk, the masks when
    // the caller's are host memory, the two key areas of the selection, and set's small block (live centres, sizes, cursors)
    DevBuf prb_cell, prb_base, prb_total, prb_mask, prb_keys_a, prb_keys_b, prb_meta;
    // distinct results (mmiss_index_query_distinct): the list stage's labels, distances and counts ([Q, pool], [Q, pool], [Q]), and the
    // suppression stage's outputs when the caller's are host memory
    DevBuf dst_list, dst_out;
    // subset search (mmiss_index_query_subset): the caller's list when it is host memory, the bitmap of one bit per row, the
    // block counts / offsets of its compaction, the listed rows in ascending order. The totals, masks and key areas are the
    // probed call's (prb_total, prb_mask, prb_keys_a / _b): both calls hold the handle's lock from their first launch to their last
    DevBuf sub_cand, sub_bitmap, sub_blk, sub_rows;
    // search after (mmiss_index_query_after): the caller's cursors and radii when they are host memory, the resolved cursors, the
    // remaining counts — one block (after_layout). The list, its compaction, the totals, masks and key areas are the subset call's
    DevBuf aft_cur;
    // grouped search (mmiss_index_set_groups, mmiss_index_query_grouped): the GROUP of every row, -1 = a group of its own, as a
    // host mirror beside tags_h; group_hwm = G, the largest group id set since the last clear or load, + 1. No kernel of any
    // other call reads groups: the device copy ([count] int32) belongs to the grouped call, which uploads it when groups_dirty
    // says the mirror changed (a set, an add, a removal, a clear, a load). Then the call's scratch: the list stage's lists, the
    // outputs on their way to host buffers and the exhaustive route's [chunk, k] results, the flagged queries; the walk's flags
    // arrive in a pinned block of its own. Totals, masks and key areas are the probed call's, as for the subset call.
    std::vector<int32_t> groups_h;
    int64_t group_hwm = 0;
    bool groups_dirty = true;
    DevBuf grp_col, grp_list, grp_out, grp_sel, grp_map;
    PinBuf grp_pin;
    hipStream_t stream() const { return has_user_stream ? user_stream : own_stream; }
};

// every other entry point refuses to run between query_begin and query_end (the scratch buffers belong to that query)
#define MM_NO_PENDING(ix, who) \
    do { if ((ix)->pend.active) MM_FAIL(MMISS_ERR_STATE, "%s: a query begun with mmiss_index_query_begin is still open", who); } while (0)

namespace {

// The element types of an index's storage dtype: T the rows as the kernels read them, Q the first pass's query operand (f16
// for f16 and fp8 rows), Bits the type a row element is moved as. with_storage() is the one place a dtype becomes types; it
// returns f(Storage<..>{}) for `dtype`.
template <typename T_, typename Q_, typename Bits_> struct Storage { using T = T_; using Q = Q_; using Bits = Bits_; };
template <typename F> auto with_storage(int dtype, F&& f) {
    if (dtype == MMISS_F16) return f(Storage<_Float16, _Float16, _Float16>{});
    if (dtype == MMISS_F8) return f(Storage<F8, _Float16, uint8_t>{});
    return f(Storage<float, float, float>{});
}
template <typename S> constexpr bool is_f8 = std::is_same<typename S::T, F8>::value;

// A set of the four per-row buffers for `cap` rows. Inverse norms (fp8 rows only) and tags are zero behind the rows: the score
// GEMM reads the inverse norms of a whole 256-row tile, the scan the tags and inverse norms of a 16-row one.
struct RowStore {
    DevBuf rows, labels, inv, tags;
    int alloc(const mmiss_index* ix, int64_t cap, hipStream_t st) {
        MM_TRY(rows.alloc((size_t)cap * ix->dim * ix->elt));
        MM_TRY(labels.alloc((size_t)cap * 8));
        MM_TRY(tags.alloc((size_t)cap * 8));
        MM_HIP(hipMemsetAsync(tags.p, 0, (size_t)cap * 8, st));
        if (ix->dtype == MMISS_F8) {
            MM_TRY(inv.alloc((size_t)cap * 4));
            MM_HIP(hipMemsetAsync(inv.p, 0, (size_t)cap * 4, st));
        }
        return MMISS_OK;
    }
};

// the index's row buffers and `s` trade places (the old ones leave with `s`)
void swap_rows(mmiss_index* ix, RowStore& s) { ix->rows.swap(s.rows); ix->labels_d.swap(s.labels); ix->inv.swap(s.inv); ix->tags.swap(s.tags); }

// Forget the partition of a partitioned search (update, remove, clear, load: rows move or change, and a stale cell would silently
// lose results). Every partition call returns with its work finished, so nothing queued reads these buffers.
void drop_partition(mmiss_index* ix) {
    mmiss_index::Partition& p = ix->part;
    p.C = 0; p.B = p.in_cells = p.largest = p.empty = p.queries = p.scanned = 0;
    p.cn.release(); p.cells.release(); p.order.release(); p.off.release();
    p.sizes.clear(); p.top_prefix.clear();
}

// Empty the index: no rows, and inverse norms and tags zero up to capacity (the invariant behind `count`); returns drained.
int reset_rows(mmiss_index* ix, hipStream_t st) {
    drop_partition(ix);
    ix->count = 0;
    ix->labels_h.clear();
    ix->tags_h.clear();
    ix->groups_h.clear(); ix->group_hwm = 0; ix->groups_dirty = true;
    if (ix->capacity == 0) return MMISS_OK;
    if (ix->dtype == MMISS_F8) MM_HIP(hipMemsetAsync(ix->inv.p, 0, (size_t)ix->capacity * 4, st));
    MM_HIP(hipMemsetAsync(ix->tags.p, 0, (size_t)ix->capacity * 8, st));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

int index_reserve(mmiss_index* ix, int64_t need, hipStream_t st) {
    if (need <= ix->capacity) return MMISS_OK;
    int64_t cap = ix->capacity > 0 ? ix->capacity : 1024;
    while (cap < need) cap *= 2;
    RowStore fresh;
    MM_TRY(fresh.alloc(ix, cap, st));
    if (ix->count > 0) {
        MM_HIP(hipMemcpyAsync(fresh.rows.p, ix->rows.p, (size_t)ix->count * ix->dim * ix->elt, hipMemcpyDeviceToDevice, st));
        MM_HIP(hipMemcpyAsync(fresh.labels.p, ix->labels_d.p, (size_t)ix->count * 8, hipMemcpyDeviceToDevice, st));
        if (fresh.inv.p) MM_HIP(hipMemcpyAsync(fresh.inv.p, ix->inv.p, (size_t)ix->count * 4, hipMemcpyDeviceToDevice, st));
        MM_HIP(hipMemcpyAsync(fresh.tags.p, ix->tags.p, (size_t)ix->count * 8, hipMemcpyDeviceToDevice, st));
    }
    MM_HIP(hipStreamSynchronize(st));
    swap_rows(ix, fresh);
    ix->capacity = cap;
    return MMISS_OK;
}

// the inverse norms of fp8 rows [row0, row0 + n) from their codes (after every write of rows: add, update, load)
int launch_f8_inv(mmiss_index* ix, int64_t row0, int64_t n, hipStream_t st) {
    if (n <= 0 || ix->dtype != MMISS_F8) return MMISS_OK;
    hipLaunchKernelGGL(f8_row_inv_kernel, dim3((int)((n + 3) / 4)), dim3(256), 0, st, ix->rows.as<uint8_t>() + (size_t)row0 * ix->dim, n,
                       ix->dim, ix->inv.as<float>() + row0);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// `row0`: the index row dst stands for (fp8 rows: where the inverse norms go)
int launch_normalize(mmiss_index* ix, const float* src_dev, void* dst, int64_t n, hipStream_t st, int64_t row0) {
    if (n <= 0) return MMISS_OK;
    MM_PROF("normalize_rows", st, 4.0 * n * ix->dim, (double)n * ix->dim * (4 + ix->elt));
    with_storage(ix->dtype, [&](auto s) {
        using T = typename decltype(s)::T;
        hipLaunchKernelGGL(normalize_rows_kernel<T>, dim3((int)((n + 3) / 4)), dim3(256), 0, st, src_dev, (T*)dst, n, ix->dim);
    });
    MM_HIP(hipGetLastError());
    return launch_f8_inv(ix, row0, n, st);   // (fp8 rows only)
}

// ---- the movers of host-or-device arrays
// n bytes from src (host or device) to dst (host or device), queued on st
int copy_any(void* dst, const void* src, size_t n, hipStream_t st) {
    if (n == 0) return MMISS_OK;
    const bool sd = mmiss_is_device_ptr(src), dd = mmiss_is_device_ptr(dst);
    if (!sd && !dd) { memcpy(dst, src, n); return MMISS_OK; }
    MM_HIP(hipMemcpyAsync(dst, src, n, sd ? (dd ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost) : hipMemcpyHostToDevice, st));
    return MMISS_OK;
}

// n zero bytes to dst (host or device, may be null); device memory on st and, `wait`, waited for
int zero_any(void* dst, size_t n, hipStream_t st, bool wait) {
    if (!dst || n == 0) return MMISS_OK;
    if (!mmiss_is_device_ptr(dst)) { memset(dst, 0, n); return MMISS_OK; }
    MM_HIP(hipMemsetAsync(dst, 0, n, st));
    if (wait) MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// host copy of a (host or device) array of n V. Device memory is read on *st and waited for; st == nullptr: by a blocking copy
// on the default stream (the labels of the mutating calls)
template <typename V> int fetch_host(const V* p, int64_t n, std::vector<V>& out, const hipStream_t* st = nullptr) {
    out.resize((size_t)n);
    if (n == 0) return MMISS_OK;
    if (!mmiss_is_device_ptr(p)) {
        memcpy(out.data(), p, (size_t)n * sizeof(V));
    } else if (!st) {
        MM_HIP(hipMemcpy(out.data(), p, (size_t)n * sizeof(V), hipMemcpyDeviceToHost));
    } else {
        MM_HIP(hipMemcpyAsync(out.data(), p, (size_t)n * sizeof(V), hipMemcpyDeviceToHost, *st));
        MM_HIP(hipStreamSynchronize(*st));
    }
    return MMISS_OK;
}

// *p as the kernels can read it: itself when it is null or device memory, else its n elements copied into `buf` at byte `at`
// (queued on st); `buf` holds `total` bytes by then
template <typename V> int device_view(const V** p, size_t n, DevBuf& buf, size_t at, size_t total, hipStream_t st) {
    if (!*p || mmiss_is_device_ptr(*p)) return MMISS_OK;
    MM_TRY(buf.ensure(total));
    V* const d = reinterpret_cast<V*>(buf.as<char>() + at);
    MM_HIP(hipMemcpyAsync(d, *p, n * sizeof(V), hipMemcpyHostToDevice, st));
    *p = d;
    return MMISS_OK;
}

// are a call's outputs (cnt and opt may be null) all host or all device memory? *dev: which
int outputs_all_host_or_all_device(const char* who, const void* lab, const void* dist, const void* cnt, const void* opt, bool* dev) {
    *dev = mmiss_is_device_ptr(lab);
    if (*dev != mmiss_is_device_ptr(dist) || (cnt && *dev != mmiss_is_device_ptr(cnt)) || (opt && *dev != mmiss_is_device_ptr(opt)))
        MM_FAIL(MMISS_ERR_ARG, "%s: output pointers must be all host or all device", who);
    return MMISS_OK;
}

// what an entry does under the lock before it touches the device: no query open, the handle's device current; *st: its stream
int enter(mmiss_index* ix, const char* who, hipStream_t* st) {
    MM_NO_PENDING(ix, who);
    MM_TRY(mmiss_use_device(ix->device));
    *st = ix->stream();
    return MMISS_OK;
}

PlanOptions plan_options() {
    PlanOptions o;
    o.scan_rounds = mmiss_option("scan_rounds", o.scan_rounds); o.scan_max_slabs = mmiss_option("scan_max_slabs", o.scan_max_slabs);
    o.merge_two_level_min = mmiss_option("merge_two_level_min", o.merge_two_level_min);
    o.score_strip_fit = mmiss_option("score_strip_fit", o.score_strip_fit); o.score_strip = mmiss_option("score_strip", o.score_strip);
    o.probe_scratch_kb = mmiss_option("probe_scratch_kb", o.probe_scratch_kb);
    return o;
}

inline bool tag_admits_h(uint64_t tag, uint64_t req, uint64_t exc) { return (tag & req) == req && (tag & exc) == 0; }

int64_t find_row(const mmiss_index* ix, int64_t label) {
    auto it = std::lower_bound(ix->labels_h.begin(), ix->labels_h.end(), label);
    if (it == ix->labels_h.end() || *it != label) return -1;
    return it - ix->labels_h.begin();
}

// The one map from a scan plan to its kernel: list mode keeps 64 entries per query and wave in a 16-query tile and 32 in the
// wider ones (plan_scan's cap), threshold mode 32 in all; rows in groups of 8, or of 16 for unfiltered f16 lists of a 16-query
// tile with scan_group = 16. FILT: a filtered query (mmiss_index_query_filtered), the same plans.
typedef void (*ScanKernel)(ScanArgs);
template <typename T, bool THR, bool FILT>
ScanKernel scan_kernel(const ScanPlan& p) {
    if (p.nqt == 4) return &scan_topk_kernel<T, 4, 32, 8, THR, FILT>;
    if (p.nqt == 2) return &scan_topk_kernel<T, 2, 32, 8, THR, FILT>;
    if constexpr (std::is_same<T, _Float16>::value && !THR && !FILT)
        if (mmiss_option("scan_group", 8) == 16) return &scan_topk_kernel<T, 1, 64, 16, false, false>;
    return &scan_topk_kernel<T, 1, THR ? 32 : 64, 8, THR, FILT>;
}

int launch_scan(mmiss_index* ix, hipStream_t st, const ScanArgs& a, const ScanPlan& p) {
    // (threshold mode: every query tile reads the whole index)
    const double flops = 2.0 * a.Q * (double)a.N * a.D;
    const double bytes = (p.thr ? (double)p.qtiles : 1.0) * a.N * a.D * ix->elt;
    const bool f16 = ix->dtype == MMISS_F16, f8 = ix->dtype == MMISS_F8;
    MM_PROF(p.thr ? (f16 ? "sweep_scan_f16" : f8 ? "sweep_scan_f8" : "sweep_scan_f32")
                  : (f16 ? "scan_topk_f16" : f8 ? "scan_topk_f8" : "scan_topk_f32"), st, flops, bytes);
    const ScanKernel kern = with_storage(ix->dtype, [&](auto s) {
        using T = typename decltype(s)::T;
        if (p.thr) return a.tags ? scan_kernel<T, true, true>(p) : scan_kernel<T, true, false>(p);
        return a.tags ? scan_kernel<T, false, true>(p) : scan_kernel<T, false, false>(p);
    });
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), p.lds));
    hipLaunchKernelGGL(kern, dim3(p.slabs, p.qtiles), dim3(256), p.lds, st, a);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

int launch_merge(mmiss_index* ix, hipStream_t st, MergeArgs m) {
    if (merge_two_level(m.L, plan_options())) {
        const int per = MERGE_LISTS_PER_BLOCK;
        const int S = (m.L + per - 1) / per;
        MM_TRY(ix->lists2_s.ensure((size_t)S * m.Q * m.kp * 4));
        MM_TRY(ix->lists2_r.ensure((size_t)S * m.Q * m.kp * 4));
        MergeArgs m1 = m;
        m1.lists_per_block = per; m1.out_s = ix->lists2_s.as<float>(); m1.out_r = ix->lists2_r.as<int32_t>();
        m1.cur_s = nullptr; m1.cur_r = nullptr;
        {
            MM_PROF("merge_lists", st, 0.0, (double)m.L * m.Q * m.kp * 8);
            hipLaunchKernelGGL(merge_lists_kernel, dim3(m.Q, S), dim3(256), 0, st, m1);
            MM_HIP(hipGetLastError());
        }
        m.in_s = ix->lists2_s.as<float>(); m.in_r = ix->lists2_r.as<int32_t>(); m.L = S;
    }
    m.lists_per_block = 0; m.out_s = nullptr; m.out_r = nullptr;
    MM_PROF("merge_lists", st, 0.0, (double)m.L * m.Q * m.kp * 8);
    hipLaunchKernelGGL(merge_lists_kernel, dim3(m.Q), dim3(256), 0, st, m);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// the handle's streams and its event (those that exist), then the handle: destroy, and every failure path of create
void release_handle(mmiss_index* ix) {
    if (ix->own_stream) (void)hipStreamDestroy(ix->own_stream);
    if (ix->side_stream) (void)hipStreamDestroy(ix->side_stream);
    if (ix->done_ev) (void)hipEventDestroy(ix->done_ev);
    delete ix;
}

}  // namespace

// ================================================================================================ lifecycle
extern "C" int mmiss_index_create(int32_t dim, int32_t storage_dtype, int device, int64_t capacity_hint,
                                  mmiss_index** out) {
    if (!out) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_create: null out");
    if (dim <= 0 || dim % 128 || dim > 4096) MM_FAIL(MMISS_ERR_UNSUPPORTED, "index dim %d: need a multiple of 128, <= 4096", dim);
    if (storage_dtype != MMISS_F32 && storage_dtype != MMISS_F16 && storage_dtype != MMISS_F8)
        MM_FAIL(MMISS_ERR_ARG, "unknown storage dtype %d", storage_dtype);
    // the streaming scan stages 16 queries in the storage's query dtype (f32 rows: f32 queries) beside its lists: f32 rows
    // fit up to dim 1920, f16 / fp8 rows up to 3968 (a create-time answer instead of a failed launch at the first query)
    if (scan_lds_bytes(dim, storage_dtype == MMISS_F32 ? 4 : 2, 1, 64) > SCAN_LDS_LIMIT)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "index dim %d with storage dtype %d: a 16-query block of the scan needs %d bytes of LDS (limit %d); "
                "f32 rows go up to dim 1920, f16 / fp8 rows up to 3968", dim, storage_dtype,
                scan_lds_bytes(dim, storage_dtype == MMISS_F32 ? 4 : 2, 1, 64), SCAN_LDS_LIMIT);
    MM_TRY(mmiss_use_device(device));
    mmiss_index* ix = new (std::nothrow) mmiss_index();
    if (!ix) MM_FAIL(MMISS_ERR_NOMEM, "out of host memory");
    ix->dim = dim; ix->dtype = storage_dtype; ix->device = device; ix->elt = storage_dtype == MMISS_F16 ? 2 : storage_dtype == MMISS_F8 ? 1 : 4;
    if (hipStreamCreateWithFlags(&ix->own_stream, hipStreamNonBlocking) != hipSuccess) {
        release_handle(ix);
        MM_FAIL(MMISS_ERR_HIP, "hipStreamCreate failed");
    }
    // The LOWEST stream priority, and not for the scheduling: the pipelined step measures the same at either priority
    // (profiles/query_side_stream.txt). The runtime deals a process's streams onto a few hardware queues PER PRIORITY (4 by
    // default); a normal-priority side stream shared its queue with one caller's stream in four, and packets of one queue are
    // taken in order, so query_end then waited for everything the caller had queued behind query_begin after all. Callers'
    // streams are normal priority as a rule (torch's default and pool streams are), so this one never shares with them.
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_lo = 0;
    if (hipStreamCreateWithPriority(&ix->side_stream, hipStreamNonBlocking, prio_lo) != hipSuccess) {
        release_handle(ix);
        MM_FAIL(MMISS_ERR_HIP, "hipStreamCreate failed");
    }
    if (hipEventCreateWithFlags(&ix->done_ev, hipEventDisableTiming) != hipSuccess) {
        release_handle(ix);
        MM_FAIL(MMISS_ERR_HIP, "hipEventCreate failed");
    }
    if (capacity_hint > 0) {
        int rc = index_reserve(ix, capacity_hint, ix->own_stream);
        if (rc != MMISS_OK) {
            release_handle(ix);
            return rc;
        }
    }
    *out = ix;
    return MMISS_OK;
}

extern "C" int mmiss_index_destroy(mmiss_index* ix) {
    if (!ix) return MMISS_OK;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    release_handle(ix);
    return MMISS_OK;
}

extern "C" int mmiss_index_set_stream(mmiss_index* ix, void* hip_stream, int32_t use_own) {
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_index_set_stream");
    hipStream_t next = reinterpret_cast<hipStream_t>(hip_stream);
    const bool next_user = use_own == 0;
    if (next_user != ix->has_user_stream || (next_user && next != ix->user_stream)) {
        // the handle's workspaces are shared by consecutive calls: wait for what the last call left on the stream being
        // left (calls on the handle's own stream, and calls with host outputs, return drained)
        MM_TRY(mmiss_use_device(ix->device));
        if (ix->async_pending) MM_HIP(hipEventSynchronize(ix->done_ev));
        ix->async_pending = false;
    }
    ix->user_stream = next;
    ix->has_user_stream = next_user;
    return MMISS_OK;
}

extern "C" int mmiss_index_count(mmiss_index* ix, int64_t* count) {
    if (!ix || !count) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_count: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    *count = ix->count;
    return MMISS_OK;
}

extern "C" int mmiss_index_clear(mmiss_index* ix) {
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_index_clear");
    if (ix->capacity > 0) MM_TRY(mmiss_use_device(ix->device));
    return reset_rows(ix, ix->stream());
}

// ================================================================================================ mutation
extern "C" int mmiss_index_add(mmiss_index* ix, const float* vecs, const int64_t* labels, int64_t n) {
    if (!ix || (n > 0 && (!vecs || !labels))) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_add: null argument");
    if (n < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_add: n = %lld", (long long)n);
    if (n == 0) return MMISS_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_index_add", &st));
    std::vector<int64_t> lab;
    MM_TRY(fetch_host(labels, n, lab));
    int64_t prev = ix->labels_h.empty() ? INT64_MIN : ix->labels_h.back();
    for (int64_t i = 0; i < n; ++i) {
        if (lab[i] < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_add: negative label %lld", (long long)lab[i]);
        if (lab[i] <= prev)
            MM_FAIL(MMISS_ERR_ARG, "mmiss_index_add: labels must be strictly increasing (label %lld after %lld)",
                    (long long)lab[i], (long long)prev);
        prev = lab[i];
    }
    if (ix->count + n >= (int64_t)INT32_MAX - 64) MM_FAIL(MMISS_ERR_UNSUPPORTED, "index shard limited to 2^31 rows");
    MM_TRY(index_reserve(ix, ix->count + n, st));
    const int D = ix->dim;
    const bool in_dev = mmiss_is_device_ptr(vecs);
    const int64_t chunk = 1 << 16;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const float* src = vecs + r0 * D;
        if (!in_dev) {
            MM_TRY(ix->stage.ensure((size_t)chunk * D * 4));
            MM_HIP(hipMemcpyAsync(ix->stage.p, src, (size_t)nr * D * 4, hipMemcpyHostToDevice, st));
            src = ix->stage.as<float>();
        }
        MM_TRY(launch_normalize(ix, src, ix->rows.as<char>() + (size_t)(ix->count + r0) * D * ix->elt, nr, st, ix->count + r0));
        if (!in_dev) MM_HIP(hipStreamSynchronize(st));
    }
    MM_HIP(hipMemcpyAsync(ix->labels_d.as<int64_t>() + ix->count, lab.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    MM_HIP(hipStreamSynchronize(st));
    ix->labels_h.insert(ix->labels_h.end(), lab.begin(), lab.end());
    ix->tags_h.resize((size_t)(ix->count + n), 0);   // new rows: tag 0 (the device tags behind count are zero)
    ix->groups_h.resize((size_t)(ix->count + n), -1); ix->groups_dirty = true;   // ... and no group
    ix->count += n;
    return MMISS_OK;
}

extern "C" int mmiss_index_update(mmiss_index* ix, const int64_t* labels, const float* vecs, int64_t n) {
    if (!ix || (n > 0 && (!vecs || !labels))) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_update: null argument");
    if (n <= 0) return n == 0 ? MMISS_OK : MMISS_ERR_ARG;
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_index_update", &st));
    std::vector<int64_t> lab;
    MM_TRY(fetch_host(labels, n, lab));
    std::vector<int64_t> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        rows[i] = find_row(ix, lab[i]);
        if (rows[i] < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_update: label %lld not in the index", (long long)lab[i]);
    }
    drop_partition(ix);   // (rows change)
    const int D = ix->dim;
    const float* src = vecs;
    MM_TRY(device_view(&src, (size_t)n * D, ix->stage, 0, (size_t)n * D * 4, st));
    for (int64_t i = 0; i < n; ++i)
        MM_TRY(launch_normalize(ix, src + i * D, ix->rows.as<char>() + (size_t)rows[i] * D * ix->elt, 1, st, rows[i]));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

extern "C" int mmiss_index_remove(mmiss_index* ix, const int64_t* labels, int64_t n, int64_t* removed) {
    if (!ix || (n > 0 && !labels)) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_remove: null argument");
    if (removed) *removed = 0;
    if (n <= 0) return n == 0 ? MMISS_OK : MMISS_ERR_ARG;
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_index_remove", &st));
    std::vector<int64_t> lab;
    MM_TRY(fetch_host(labels, n, lab));
    std::vector<char> drop((size_t)ix->count, 0);
    int64_t ndrop = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = find_row(ix, lab[i]);
        if (r >= 0 && !drop[r]) { drop[r] = 1; ++ndrop; }
    }
    if (removed) *removed = ndrop;
    if (ndrop == 0) return MMISS_OK;
    drop_partition(ix);   // (rows move)
    const int64_t keep = ix->count - ndrop;
    if (keep == 0) return reset_rows(ix, st);   // every row removed
    std::vector<int64_t> map((size_t)keep), nl((size_t)keep);
    std::vector<uint64_t> ntag((size_t)keep);
    std::vector<int32_t> ngrp((size_t)keep);
    for (int64_t r = 0, o = 0; r < ix->count; ++r)
        if (!drop[r]) { map[o] = r; nl[o] = ix->labels_h[r]; ntag[o] = ix->tags_h[r]; ngrp[o] = ix->groups_h[r]; ++o; }
    // stable compaction into fresh buffers (row order == label order is the tie-break contract)
    RowStore fresh;
    MM_TRY(fresh.alloc(ix, ix->capacity, st));
    MM_HIP(hipMemcpyAsync(fresh.tags.p, ntag.data(), (size_t)keep * 8, hipMemcpyHostToDevice, st));   // (the host mirror, compacted)
    MM_TRY(ix->map.ensure((size_t)keep * 8));
    MM_HIP(hipMemcpyAsync(ix->map.p, map.data(), (size_t)keep * 8, hipMemcpyHostToDevice, st));
    with_storage(ix->dtype, [&](auto s) {
        using B = typename decltype(s)::Bits;
        hipLaunchKernelGGL(gather_rows_kernel<B>, dim3((int)std::min<int64_t>(4096, (keep * ix->dim + 255) / 256)), dim3(256), 0, st,
                           ix->rows.as<B>(), ix->map.as<int64_t>(), fresh.rows.as<B>(), keep, ix->dim);
        if constexpr (is_f8<decltype(s)>)
            hipLaunchKernelGGL(gather_rows_kernel<float>, dim3((int)std::min<int64_t>(4096, (keep + 255) / 256)), dim3(256), 0, st,
                               ix->inv.as<float>(), ix->map.as<int64_t>(), fresh.inv.as<float>(), keep, 1);
    });
    MM_HIP(hipGetLastError());
    MM_HIP(hipMemcpyAsync(fresh.labels.p, nl.data(), (size_t)keep * 8, hipMemcpyHostToDevice, st));
    MM_HIP(hipStreamSynchronize(st));
    swap_rows(ix, fresh);
    ix->labels_h.swap(nl);
    ix->tags_h.swap(ntag);
    ix->groups_h.swap(ngrp); ix->groups_dirty = true;
    ix->count = keep;
    return MMISS_OK;
}

extern "C" int mmiss_index_get(mmiss_index* ix, const int64_t* labels, int64_t n, float* out) {
    if (!ix || (n > 0 && (!labels || !out))) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_get: null argument");
    if (n <= 0) return n == 0 ? MMISS_OK : MMISS_ERR_ARG;
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_index_get", &st));
    std::vector<int64_t> lab;
    MM_TRY(fetch_host(labels, n, lab));
    std::vector<int64_t> map((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        map[i] = find_row(ix, lab[i]);
        if (map[i] < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_get: label %lld not in the index", (long long)lab[i]);
    }
    MM_TRY(ix->map.ensure((size_t)n * 8));
    MM_HIP(hipMemcpyAsync(ix->map.p, map.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    const bool out_dev = mmiss_is_device_ptr(out);
    float* dst = out;
    if (!out_dev) { MM_TRY(ix->stage.ensure((size_t)n * ix->dim * 4)); dst = ix->stage.as<float>(); }
    const int grid = (int)std::min<int64_t>(4096, (n * ix->dim + 255) / 256);
    with_storage(ix->dtype, [&](auto s) {
        using T = typename decltype(s)::T;
        if constexpr (is_f8<decltype(s)>)   // the vectors the rows represent: values x inverse norm
            hipLaunchKernelGGL(gather_rows_f8_f32_kernel, dim3(grid), dim3(256), 0, st, ix->rows.as<F8>(), ix->inv.as<float>(),
                               ix->map.as<int64_t>(), dst, n, ix->dim);
        else
            hipLaunchKernelGGL(gather_rows_f32_kernel<T>, dim3(grid), dim3(256), 0, st, ix->rows.as<T>(), ix->map.as<int64_t>(), dst,
                               n, ix->dim);
    });
    MM_HIP(hipGetLastError());
    if (!out_dev) MM_HIP(hipMemcpyAsync(out, dst, (size_t)n * ix->dim * 4, hipMemcpyDeviceToHost, st));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

extern "C" int mmiss_index_labels(mmiss_index* ix, int64_t* out, int64_t cap) {
    if (!ix || (!out && cap > 0)) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_labels: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    const int64_t n = std::min<int64_t>(cap, ix->count);
    if (n > 0) memcpy(out, ix->labels_h.data(), (size_t)n * 8);
    return MMISS_OK;
}

// ================================================================================================ tags (filtered queries)
extern "C" int mmiss_index_set_tags(mmiss_index* ix, const int64_t* labels, const uint64_t* tags, int64_t n) {
    if (!ix || (n > 0 && (!labels || !tags))) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_set_tags: null argument");
    if (n < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_set_tags: n = %lld", (long long)n);
    if (n == 0) return MMISS_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_index_set_tags", &st));
    std::vector<int64_t> lab;
    std::vector<uint64_t> val;
    MM_TRY(fetch_host(labels, n, lab));
    MM_TRY(fetch_host(tags, n, val, &st));
    std::vector<int64_t> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {   // every label first: a missing one changes nothing
        rows[i] = find_row(ix, lab[i]);
        if (rows[i] < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_set_tags: label %lld not in the index", (long long)lab[i]);
    }
    // the host mirror in call order (a label given twice keeps its last tag), then its values for the distinct rows to the device
    std::vector<uint64_t>& mirror = ix->tags_h;
    for (int64_t i = 0; i < n; ++i) mirror[(size_t)rows[i]] = val[i];
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    const int64_t m = (int64_t)rows.size();
    std::vector<uint64_t> pack((size_t)m * 2);
    for (int64_t i = 0; i < m; ++i) { pack[i] = (uint64_t)rows[i]; pack[m + i] = mirror[(size_t)rows[i]]; }
    MM_TRY(ix->tag_stage.ensure((size_t)m * 16));
    MM_HIP(hipMemcpyAsync(ix->tag_stage.p, pack.data(), (size_t)m * 16, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(scatter_u64_kernel, dim3((int)std::min<int64_t>(4096, (m + 255) / 256)), dim3(256), 0, st,
                       ix->tags.as<uint64_t>(), ix->tag_stage.as<int64_t>(), ix->tag_stage.as<uint64_t>() + m, m);
    MM_HIP(hipGetLastError());
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

extern "C" int mmiss_index_get_tags(mmiss_index* ix, const int64_t* labels, int64_t n, uint64_t* out) {
    if (!ix || (n > 0 && (!labels || !out))) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_get_tags: null argument");
    if (n <= 0) return n == 0 ? MMISS_OK : MMISS_ERR_ARG;
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_index_get_tags");
    std::vector<int64_t> lab;
    MM_TRY(fetch_host(labels, n, lab));
    std::vector<uint64_t> val((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = find_row(ix, lab[i]);
        if (r < 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_get_tags: label %lld not in the index", (long long)lab[i]);
        val[i] = ix->tags_h[(size_t)r];
    }
    if (mmiss_is_device_ptr(out)) {
        MM_TRY(mmiss_use_device(ix->device));
        MM_HIP(hipMemcpyAsync(out, val.data(), (size_t)n * 8, hipMemcpyHostToDevice, ix->stream()));
        MM_HIP(hipStreamSynchronize(ix->stream()));
    } else {
        memcpy(out, val.data(), (size_t)n * 8);
    }
    return MMISS_OK;
}

// ================================================================================================ groups (grouped search)
extern "C" int mmiss_index_set_groups(mmiss_index* ix, const int64_t* labels, const int32_t* groups, int64_t n) {
    const char* who = "mmiss_index_set_groups";
    if (!ix || (n > 0 && (!labels || !groups))) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (n < 0) MM_FAIL(MMISS_ERR_ARG, "%s: n = %lld", who, (long long)n);
    if (n == 0) return MMISS_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    std::vector<int64_t> lab;
    std::vector<int32_t> val;
    MM_TRY(fetch_host(labels, n, lab));
    MM_TRY(fetch_host(groups, n, val, &st));
    std::vector<int64_t> rows((size_t)n);
    int32_t top = -1;
    for (int64_t i = 0; i < n; ++i) {   // every label and value first: a bad one changes nothing
        rows[i] = find_row(ix, lab[i]);
        if (rows[i] < 0) MM_FAIL(MMISS_ERR_ARG, "%s: label %lld not in the index", who, (long long)lab[i]);
        if (val[i] < -1 || val[i] >= MMISS_MAX_GROUPS)
            MM_FAIL(MMISS_ERR_ARG, "%s: group %d of label %lld outside -1 .. %d", who, val[i], (long long)lab[i], MMISS_MAX_GROUPS - 1);
        top = std::max(top, val[i]);
    }
    for (int64_t i = 0; i < n; ++i) ix->groups_h[(size_t)rows[i]] = val[i];   // call order: a label given twice keeps its last group
    ix->group_hwm = std::max<int64_t>(ix->group_hwm, (int64_t)top + 1);
    ix->groups_dirty = true;   // (the device column is the grouped call's: uploaded there)
    return MMISS_OK;
}

extern "C" int mmiss_index_get_groups(mmiss_index* ix, const int64_t* labels, int64_t n, int32_t* out) {
    const char* who = "mmiss_index_get_groups";
    if (!ix || (n > 0 && (!labels || !out))) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (n <= 0) return n == 0 ? MMISS_OK : MMISS_ERR_ARG;
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    std::vector<int64_t> lab;
    MM_TRY(fetch_host(labels, n, lab));
    std::vector<int32_t> val((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = find_row(ix, lab[i]);
        if (r < 0) MM_FAIL(MMISS_ERR_ARG, "%s: label %lld not in the index", who, (long long)lab[i]);
        val[i] = ix->groups_h[(size_t)r];
    }
    if (mmiss_is_device_ptr(out)) {
        MM_TRY(mmiss_use_device(ix->device));
        MM_HIP(hipMemcpyAsync(out, val.data(), (size_t)n * 4, hipMemcpyHostToDevice, ix->stream()));
        MM_HIP(hipStreamSynchronize(ix->stream()));
    } else {
        memcpy(out, val.data(), (size_t)n * 4);
    }
    return MMISS_OK;
}

// ================================================================================================ exactness contract
// Stage 1 orders rows by APPROXIMATE scores (matrix cores, f32 accumulation, f16 query operand for f16 / fp8 rows) and keeps
// k' > k of them; stage 2 re-scores the survivors canonically (fp64, fixed order) and sorts. That is exact by construction
// only if no row left out by stage 1 can belong to the true top-k, so stage 2 PROVES it per query:
//   every left-out row r has approx(r) <= tau (tau = the k'-th approximate score / group maximum),
//   |approx(r) - canonical(r)| <= eps_q for every row (bound below), so canonical(r) <= tau + eps_q;
//   if the k-th canonical score c_k of the candidates satisfies c_k - tau > eps_q, nothing left out reaches c_k.
// A query that fails the test is WIDENED by ONE threshold pass (round 4; it used to page through the index 32 rows per
// full scan): c_k is a lower bound of the true k-th canonical score, so every row of the true top-k has
// approx >= c_k - eps_q =: thr_q. One more pass over the index — the score GEMM for many flagged queries of an f16 index, the
// streaming scan otherwise — appends EVERY row with approx >= thr_q to the query's list; the canonical re-rank of that list
// is the exact answer (rows not on it have canonical <= approx + eps_q < c_k <= true c_k: strictly behind rank k, whatever
// the tie-break). A list that overflows its capacity (a plateau: more than SWEEP_CAP rows within eps of the k-th score,
// e.g. 10^5 uploads of one placeholder image) sends the query to the exhaustive canonical pass. Exact for any data; on
// random data the test fails for about one query in 10^4, on the encoder's own embeddings (pairwise cosine 0.99) for all.
namespace {

constexpr int SWEEP_CAP = 8192;   // rows a widened query may collect (= the re-rank kernel's sort capacity)

// the guard's bound, split into what is the same for every query and the factor of the query operand's ACTUAL rounding error
// |qs - qn|_2 (prep_queries_kernel computes eps_q = fixed + cnorm * |qs - qn|_2 per query):
//   f32 accumulation of D exact products in hardware order: <= 4 D 2^-24 sum|q_d c_d| (factor 4: margin for the MFMA's
//   internal alignment / truncation) <= 4 D 2^-24 |q||c|, |q||c| <= (1 + 2^-10)^2 (f16 / f32 rows);
//   f16 / fp8 rows: the scan's query operand is f16(qn); <f16(qn) - qn, c> <= |f16(qn) - qn|_2 |c|_2 (+ D 2^-25: products
//   of subnormal-range operands); a stored fp8 row's norm is within 1.07 of 1 (three mantissa bits per component);
//   the float rounding of the canonical distance (<= 2) is 2^-23 at most.
void guard_terms(const mmiss_index* ix, double* fixed, double* cnorm) {
    const double D = ix->dim;
    // (fp8 rows: |values| x inv = 1 up to inv's own rounding; 1.07 is kept from the un-renormalised form of round 4 — it only
    // widens the bound — and the scan's multiplication by inv adds one more f32 rounding of a score <= 1.08)
    const double cn = ix->dtype == MMISS_F8 ? 1.07 : 1.0 + ldexp(1.0, -9);
    double e = 4.0 * D * ldexp(1.0, -24) * cn * (1.0 + ldexp(1.0, -9));
    if (ix->dtype != MMISS_F32) e += D * ldexp(1.0, -25) * cn;
    if (ix->dtype == MMISS_F8) e += ldexp(1.0, -23);
    *fixed = e * 1.003 + ldexp(1.0, -21);
    *cnorm = ix->dtype == MMISS_F32 ? 0.0 : cn * 1.003;
}

// radius: the radius form of the kernel (r.max_dist; mmiss_index_query_radius*)
int launch_rerank(mmiss_index* ix, hipStream_t st, const RerankArgs& r, int blocks, bool radius = false) {
    int npow = 1;
    while (npow < r.ncand) npow <<= 1;
    const int lds = npow * 8 + 16;
    MM_PROF("rerank", st, 2.0 * blocks * r.ncand * r.D, (double)blocks * r.ncand * r.D * ix->elt);
    const int threads = r.ncand >= 16 ? 1024 : 256;  // one wave per candidate row: more waves hide the gather latency
    void (*kern)(RerankArgs) = with_storage(ix->dtype, [radius](auto s) {
        using T = typename decltype(s)::T;
        return radius ? &rerank_kernel<T, true> : &rerank_kernel<T>;
    });
    if (lds > 32768) MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, st, r);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// the canonical distance of every row to query q of the call's normalised queries (ix->qn) into ix->dist_all (float [N], sized
// by the caller); queued
int launch_canonical_scan(mmiss_index* ix, hipStream_t st, int32_t q) {
    const int64_t N = ix->count;
    const int D = ix->dim;
    MM_PROF("canonical_scan", st, 2.0 * N * D, (double)N * D * ix->elt);
    const int grid = canonical_scan_grid(N);
    with_storage(ix->dtype, [&](auto s) {   // (inv: the inverse norms of fp8 rows, null for the others)
        hipLaunchKernelGGL(canonical_scan_kernel<typename decltype(s)::T>, dim3(grid), dim3(256), 0, st, ix->rows.p, N, D,
                           ix->qn.as<float>() + (size_t)q * D, ix->dist_all.as<float>(), (const float*)ix->inv.as<float>());
    });
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// ... and from there to the pinned block ix->dist_pin (sized by the caller). Returns with the stream drained.
int canonical_distances(mmiss_index* ix, hipStream_t st, int32_t q) {
    const int64_t N = ix->count;
    MM_TRY(launch_canonical_scan(ix, st, q));
    MM_HIP(hipMemcpyAsync(ix->dist_pin.p, ix->dist_all.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// Exhaustive canonical pass for the queries of `pd` listed in `which`: canonical distance of every row (canonical_scan_kernel),
// the k best by (distance, row) picked on the host (a bounded heap: O(N log k)), final ordering / labels / counts by the
// ordinary rerank kernel with "nothing was left out" (tau = -inf).
int exhaustive_queries(mmiss_index* ix, hipStream_t st, const mmiss_index::Pending& pd, const std::vector<int32_t>& which) {
    const int64_t N = ix->count;
    const int D = ix->dim, KP = 32;
    const int kk = (int)std::min<int64_t>(pd.k, N);
    const int kkpad = (int)round_up(std::max(kk, 1), KP);
    const int nq = (int)which.size();
    if (nq == 0 || N <= 0) return MMISS_OK;
    MM_TRY(ix->dist_all.ensure((size_t)N * 4));
    // the distances come back through a PINNED block (a pageable destination makes the copy synchronous and slow: ADVICE r3)
    MM_TRY(ix->dist_pin.ensure((size_t)N * 4, st));
    const float* dist = ix->dist_pin.as<float>();
    std::vector<int32_t> cand((size_t)nq * kkpad, -1);
    typedef std::pair<float, int32_t> Ent;  // (distance, row); NaN distances never enter
    for (int i = 0; i < nq; ++i) {
        const int32_t q = which[i];
        MM_TRY(canonical_distances(ix, st, q));
        std::priority_queue<Ent> heap;  // max-heap: top = the worst of the best kk so far, by (distance, row)
        // filtered query: rows it does not admit never enter (host mirror of the tags)
        const uint64_t rq = pd.filt ? pd.req[(size_t)q] : 0, rx = pd.filt ? pd.exc[(size_t)q] : 0;
        for (int64_t r = 0; r < N; ++r) {
            const float d = dist[(size_t)r];
            if (d != d) continue;
            if (pd.filt && !tag_admits_h(ix->tags_h[(size_t)r], rq, rx)) continue;
            if ((int)heap.size() < kk) heap.push(Ent(d, (int32_t)r));
            else if (Ent(d, (int32_t)r) < heap.top()) { heap.pop(); heap.push(Ent(d, (int32_t)r)); }
        }
        int32_t* c = cand.data() + (size_t)i * kkpad;
        for (size_t j = 0; !heap.empty(); ++j) { c[j] = heap.top().second; heap.pop(); }
        ix->stat_exhaustive += 1;
    }
    // ONE re-rank launch for all of them (final ordering, labels, counts): block b = query which[b], its kkpad selected rows
    MM_TRY(ix->cand2.ensure((size_t)nq * kkpad * 4));
    MM_TRY(ix->qmap.ensure((size_t)nq * 4));
    MM_HIP(hipMemcpyAsync(ix->cand2.p, cand.data(), (size_t)nq * kkpad * 4, hipMemcpyHostToDevice, st));
    MM_HIP(hipMemcpyAsync(ix->qmap.p, which.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
    RerankArgs r{};
    r.rows = ix->rows.p; r.D = D; r.inv = ix->inv.as<float>(); r.qn = ix->qn.as<float>(); r.cand = ix->cand2.as<int32_t>();
    r.cand_stride = kkpad; r.ncand = kkpad; r.group_mode = 0; r.nrows = N;
    r.labels = ix->labels_d.as<int64_t>(); r.k = pd.k;
    r.out_labels = pd.out.lab; r.out_dist = pd.out.dist; r.out_count = pd.out.cnt;
    r.qmap = ix->qmap.as<int32_t>();
    MM_TRY(launch_rerank(ix, st, r, nq));
    MM_HIP(hipStreamSynchronize(st));  // (`cand` and `which` leave scope with the caller)
    return MMISS_OK;
}

// the strip score GEMM on the staggered loop of the persistent encoder GEMM (gemm_strip_p256.h; round 3): D % 128 == 0
bool strip_v3(const mmiss_index* ix) { return mmiss_option("score_strip_v3", 1) != 0 && (ix->dim % 128) == 0 && ix->dim >= 256; }

// the rows the strip score GEMM serves: f16, and fp8 unless score_f8_gemm = 0 (round 4: gemm256s_kernel<_Float16, .., W8>
// widens the codes to f16 in its operand load)
bool strip_gemm_rows(const mmiss_index* ix) {
    return ix->dtype == MMISS_F16 || (ix->dtype == MMISS_F8 && mmiss_option("score_f8_gemm", 1) != 0);
}

// the strip score GEMM of M queries `qs` against the index's first N rows: fp8 rows in the W8 form, f16 rows on the staggered
// loop or, v3 = false, on the strip kernel of gemm_bf16_256.h
int launch_strip_gemm(mmiss_index* ix, hipStream_t st, bool v3, const void* qs, const GemmEpi& ep, int M, int N, int strip,
                      const StripFilter* flt) {
    if (ix->dtype == MMISS_F8) return launch_gemm256s<_Float16, true>(st, qs, ix->rows.p, ep, M, N, ix->dim, strip, flt);
    if (v3) return launch_gemm256s<_Float16>(st, qs, ix->rows.p, ep, M, N, ix->dim, strip, flt);
    return launch_gemm256_strip<_Float16>(st, qs, ix->rows.p, ep, M, N, ix->dim, strip, flt);
}

// the widen pass's threshold pass over the index for Qf flagged queries: the strip score GEMM (true) or the streaming scan
// (see sweep_queries)
bool sweep_uses_gemm(const mmiss_index* ix, bool filt, int Qf) {
    return !filt && strip_gemm_rows(ix) && strip_v3(ix) && Qf > mmiss_option("sweep_gemm_min_q", 64);
}

// ONE threshold pass over the index for Qf queries: every row whose approximate score reaches its query's threshold thr_sw[q]
// is appended to the query's list ix->swp_list[q] (SWEEP_CAP entries; ix->swp_cnt[q] counts them and may run past that). The
// strip score GEMM for an f16 / fp8 index once the queries fill a quarter of a 256-query tile (it costs about what 1.2 streaming
// scans cost, and a scan serves 64 queries), the scan otherwise. fm_sw: the masks of filtered queries ([Qf] required, then [Qf]
// excluded; null: unfiltered) — always the scan, whose FILT form collects admitted rows only; the score GEMM has no filtered
// epilogue. qs_sw: [Qf rounded up to 256][D] scan operand, rows >= Qf zero; thr_sw likewise, +inf (or anything: m_valid masks
// them) behind Qf. row_begin: no query wants a row below it (the GEMM starts at its column tile). *pages: the passes over the
// index this cost. The widen pass of a top-k query and a radius query share it.
int threshold_pass(mmiss_index* ix, hipStream_t st, int Qf, const void* qs_sw, const float* thr_sw, const uint64_t* fm_sw,
                   int64_t row_begin, int* pages) {
    const int D = ix->dim;
    const int64_t N = ix->count;
    const bool gemm = sweep_uses_gemm(ix, fm_sw != nullptr, Qf);
    const int Qfp = (int)round_up(Qf, 256);
    MM_TRY(ix->swp_cnt.ensure((size_t)Qfp * 4));
    MM_TRY(ix->swp_list.ensure((size_t)Qf * SWEEP_CAP * 4));
    MM_HIP(hipMemsetAsync(ix->swp_cnt.p, 0, (size_t)Qfp * 4, st));
    *pages = 0;
    if (N <= 0) return MMISS_OK;   // (an empty index: every list stays empty)
    if (gemm) {
        const int64_t Npad = round_up(N, 256), nbn = Npad / 256;
        GemmEpi ep{};
        ep.m_valid = Qf; ep.p0 = (int)N; ep.m_fast = 1;
        ep.aux = ix->inv.as<float>();   // (fp8 rows: inverse norms; null otherwise)
        StripFilter flt{};
        flt.tau = thr_sw; flt.tau_stride = 1; flt.cnt = ix->swp_cnt.as<int32_t>();
        flt.buf_s = nullptr; flt.buf_g = ix->swp_list.as<int32_t>(); flt.cap = SWEEP_CAP;
        flt.bn_begin = (int)(std::min<int64_t>(std::max<int64_t>(row_begin, 0), N - 1) / 256);
        const int strip = strip_length(Qfp, nbn, nbn - flt.bn_begin, plan_options());
        MM_PROF(ix->dtype == MMISS_F8 ? "sweep_gemm_f8" : "sweep_gemm_f16", st, 2.0 * Qf * (double)N * D, (double)N * D * ix->elt);
        MM_TRY(launch_strip_gemm(ix, st, true, qs_sw, ep, Qfp, (int)Npad, strip, &flt));
        *pages = 1;
    } else {
        const ScanPlan p = plan_dense(D, ix->qelt(), Qf, N, false).as_scan();
        if (p.lds > SCAN_LDS_LIMIT)
            MM_FAIL(MMISS_ERR_UNSUPPORTED, "widen pass: a 16-query block of dim %d does not fit the LDS (%d bytes)", D, p.lds);
        ScanArgs a{};
        a.rows = ix->rows.p; a.N = N; a.D = D; a.inv = ix->inv.as<float>(); a.qs = qs_sw; a.Q = Qf;
        a.thr = thr_sw; a.gcnt = ix->swp_cnt.as<int32_t>(); a.glist = ix->swp_list.as<int32_t>(); a.gcap = SWEEP_CAP;
        if (fm_sw) { a.tags = ix->tags.as<uint64_t>(); a.req = fm_sw; a.exc = fm_sw + Qf; }
        a.tiles_per_block = p.tiles_per_block;
        MM_TRY(launch_scan(ix, st, a, p));
        *pages = p.qtiles;
    }
    return MMISS_OK;
}

// The canonical re-rank of the lists a threshold pass collected, Qf blocks (block b: list b; its query r.qmap[b], null: b;
// `which`: the same map on the host). `r` carries the queries, k, the outputs and, `radius`, the cut. The typical list is short
// (tens to hundreds of rows), so the first launch sorts at most SWEEP_FAST rows per query WITHOUT waiting to learn the counts;
// the counts come back with it (one wait), and only the queries that collected more get a second, larger launch. `over`: the
// blocks whose list overflowed SWEEP_CAP — theirs is the exhaustive pass, the caller's. Returns with the stream drained of the
// first launch; the second may still be queued.
int rerank_swept(mmiss_index* ix, hipStream_t st, RerankArgs r, int Qf, const int32_t* which, bool radius, std::vector<int32_t>& over) {
    const int SWEEP_FAST = 1024;
    r.rows = ix->rows.p; r.D = ix->dim; r.inv = ix->inv.as<float>(); r.qn = ix->qn.as<float>(); r.cand = ix->swp_list.as<int32_t>();
    r.cand_stride = SWEEP_CAP; r.ncand = SWEEP_FAST; r.cand_cnt = ix->swp_cnt.as<int32_t>();
    r.group_mode = 0; r.nrows = ix->count;
    r.labels = ix->labels_d.as<int64_t>();
    // the list lengths come back with the re-rank itself: every block stores its list's raw length into a pinned block (a copy
    // into pageable memory behind the kernel was a second operation and a staged host copy in front of the next query's first
    // launch: part of the ~87 us the GPU idled per pipelined step, round 6)
    MM_TRY(ix->swp_pin.ensure((size_t)Qf * 4, st, (size_t)(Qf < 1024 ? 1024 : 2 * Qf) * 4));
    r.cnt_host = ix->swp_pin.as<int32_t>();
    MM_TRY(launch_rerank(ix, st, r, Qf, radius));
    r.cnt_host = nullptr;
    MM_HIP(hipStreamSynchronize(st));
    const int32_t* cnt = ix->swp_pin.as<int32_t>();
    std::vector<int32_t> big_b;   // blocks that need the large re-rank
    int maxc = 1;
    over.clear();
    for (int b = 0; b < Qf; ++b) {
        if (cnt[b] > SWEEP_CAP) over.push_back(b);
        else {
            ix->stat_swept_rows += cnt[b];
            if (cnt[b] > SWEEP_FAST) { big_b.push_back(b); maxc = std::max(maxc, cnt[b]); }
        }
    }
    if (!big_b.empty()) {
        // block j of this launch = block big_b[j] of the sweep: its list and count by bmap, its query by qmap
        const int nb = (int)big_b.size();
        std::vector<int32_t> qm((size_t)nb);
        for (int j = 0; j < nb; ++j) qm[j] = which ? which[big_b[j]] : big_b[j];
        MM_TRY(ix->cand2.ensure((size_t)nb * 8));
        MM_HIP(hipMemcpyAsync(ix->cand2.p, big_b.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
        MM_HIP(hipMemcpyAsync(ix->cand2.as<int32_t>() + nb, qm.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
        MM_HIP(hipStreamSynchronize(st));
        r.ncand = (int)round_up(maxc, 32);
        r.bmap = ix->cand2.as<int32_t>();
        r.qmap = ix->cand2.as<int32_t>() + nb;
        MM_TRY(launch_rerank(ix, st, r, nb, radius));
    }
    return MMISS_OK;
}

// The widen pass for the queries of `pd` listed in `which` (original indices): ONE threshold pass over the index for all of
// them (thr_q = c_k - eps_q, left in ix->thr by the first pass's re-rank), the canonical re-rank of the rows it collected, and
// the exhaustive pass for the lists that overflowed. Results overwrite the queries' rows of pd's outputs. Returns with the
// stream drained.
int sweep_queries(mmiss_index* ix, hipStream_t st, const mmiss_index::Pending& pd, const std::vector<int32_t>& which) {
    const int Qf = (int)which.size(), D = ix->dim;
    const int64_t N = ix->count;
    if (Qf == 0 || N <= 0) return MMISS_OK;
    const int Qfp = (int)round_up(Qf, 256);
    // Every query of the call flagged (the encoder's own embeddings as the index: all of them, every call): the first pass's
    // operands are the sweep's operands — no gather, no map, nothing crosses PCIe. Otherwise the flagged queries are compacted.
    const bool all = Qf == pd.Q;
    const void* qs_sw = ix->qs.p;          // [>= Qfp rows][D] scan operand (rows >= Qf are zero or masked by thr = +inf)
    const float* thr_sw = ix->thr.as<float>();
    const int32_t* qmap_sw = nullptr;
    const uint64_t* fm_sw = pd.d_mask;     // filtered: [Qf] required, then [Qf] excluded masks, in the sweep's order
    std::vector<uint64_t> fm2;
    if (!all && pd.filt) {
        fm2.resize((size_t)Qf * 2);
        for (int i = 0; i < Qf; ++i) { fm2[i] = pd.req[(size_t)which[i]]; fm2[Qf + i] = pd.exc[(size_t)which[i]]; }
        MM_TRY(ix->fmask2.ensure((size_t)Qf * 16));
        MM_HIP(hipMemcpyAsync(ix->fmask2.p, fm2.data(), (size_t)Qf * 16, hipMemcpyHostToDevice, st));
        fm_sw = ix->fmask2.as<uint64_t>();
    }
    if (!all) {
        std::vector<int64_t> map64(which.begin(), which.end());
        MM_TRY(ix->qmap.ensure((size_t)Qf * 4));
        MM_TRY(ix->qmap64.ensure((size_t)Qf * 8));
        MM_TRY(ix->qs2.ensure((size_t)Qfp * D * ix->qelt()));
        MM_TRY(ix->thr2.ensure((size_t)Qfp * 4));
        MM_HIP(hipMemcpyAsync(ix->qmap.p, which.data(), (size_t)Qf * 4, hipMemcpyHostToDevice, st));
        MM_HIP(hipMemcpyAsync(ix->qmap64.p, map64.data(), (size_t)Qf * 8, hipMemcpyHostToDevice, st));
        MM_HIP(hipStreamSynchronize(st));   // (pageable sources: `map64` goes out of scope)
        if (Qfp > Qf) MM_HIP(hipMemsetAsync(ix->qs2.as<char>() + (size_t)Qf * D * ix->qelt(), 0, (size_t)(Qfp - Qf) * D * ix->qelt(), st));
        with_storage(ix->dtype, [&](auto s) {   // (f16 query operand for f16 and fp8 rows)
            using QT = typename decltype(s)::Q;
            hipLaunchKernelGGL(gather_rows_kernel<QT>, dim3((int)std::min<int64_t>(4096, ((int64_t)Qf * D + 255) / 256)), dim3(256), 0, st,
                               ix->qs.as<QT>(), ix->qmap64.as<int64_t>(), ix->qs2.as<QT>(), (int64_t)Qf, D);
        });
        MM_HIP(hipGetLastError());
        hipLaunchKernelGGL(gather_rows_kernel<float>, dim3((Qf + 255) / 256), dim3(256), 0, st, ix->thr.as<float>(),
                           ix->qmap64.as<int64_t>(), ix->thr2.as<float>(), (int64_t)Qf, 1);
        MM_HIP(hipGetLastError());
        qs_sw = ix->qs2.p; thr_sw = ix->thr2.as<float>(); qmap_sw = ix->qmap.as<int32_t>();
    }
    int pages = 0;
    MM_TRY(threshold_pass(ix, st, Qf, qs_sw, thr_sw, pd.filt ? fm_sw : nullptr, 0, &pages));
    ix->stat_pages += pages;
    // Re-rank what was collected; past SWEEP_CAP, the exhaustive pass.
    RerankArgs r{};
    r.k = pd.k;
    r.out_labels = pd.out.lab; r.out_dist = pd.out.dist; r.out_count = pd.out.cnt;
    r.qmap = qmap_sw;
    std::vector<int32_t> over, rest;   // blocks whose list overflowed / their original indices for the exhaustive pass
    MM_TRY(rerank_swept(ix, st, r, Qf, which.data(), false, over));
    ix->stat_rounds += 1;
    for (int32_t b : over) rest.push_back(which[b]);
    MM_TRY(exhaustive_queries(ix, st, pd, rest));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

}  // namespace

// ================================================================================================ query
namespace {

// The path of one query call, decided once from its shape and the options (plan_query).
struct QueryPlan {
    int kp = 0, pages = 0, ncand = 0;   // candidates per page (k'; groups of 16 rows on the dense path), pages of them
    bool dense = false;      // first pass: the score GEMM to group maxima, select, merge; the paged streaming scan otherwise
    bool dense8 = false;     // ... on fp8 rows
    bool big = false;        // ... in 256x256 tiles (Q >= score_big_min_q), else the 128-query tile
    bool strip_v3 = false;   // ... on the staggered loop (strip_v3())
    bool sample = false;     // ... in the threshold-filtered sample form
    int Mq = 0, strip = 1, filter_cap = 0;
    int64_t Npad = 0, nbn = 0, ns_tiles = 0, Ndense = 0;
};

int plan_query(const mmiss_index* ix, int Q, int k, bool filt, QueryPlan& p) {
    const int64_t N = ix->count;
    // effective k: never more than the rows there are
    const int64_t want = std::min<int64_t>(k, N);
    if (want <= 10) { p.kp = 16; p.pages = 1; }
    else if (want <= 24) { p.kp = 32; p.pages = 1; }
    else {
        p.kp = 32;
        p.pages = (int)((std::min<int64_t>(want + 8, N) + 31) / 32);
    }
    p.ncand = p.kp * p.pages;
    if (p.ncand > 2048) MM_FAIL(MMISS_ERR_UNSUPPORTED, "mmiss_index_query: k = %d too large (max 2040)", k);

    // batched path: f16 rows, more than one MFMA tile of queries, single page
    // ... and fp8 rows from two 128-query tiles on (round 4: below that the streaming scan, which reads half the bytes per
    // row, is the faster)
    // (filtered queries never take it: every pass of theirs is the streaming scan's FILT form)
    const bool single = !filt && N > 0 && p.pages == 1;
    p.big = Q >= mmiss_option("score_big_min_q", 129);
    p.strip_v3 = strip_v3(ix);
    p.dense8 = single && ix->dtype == MMISS_F8 && p.big && p.strip_v3 && strip_gemm_rows(ix);
    p.dense = (single && ix->dtype == MMISS_F16 && Q > 16) || p.dense8;
    if (!p.dense) return MMISS_OK;
    // 256x256 phase-pipelined tile once there are two 128-query tiles to share a row panel
    p.Npad = round_up(N, p.big ? 256 : 128);
    p.Mq = (int)round_up(Q, p.big ? 256 : 128);
    // Threshold-filtered selection (Q > 128, index of at least 128 tiles): the first 1/32 of the rows (the SAMPLE) goes
    // through the dense path — group maxima to HBM, select, merge — which yields each query's k' best sample groups and
    // their k'-th score tau_q. tau_q is a lower bound of the final k'-th best group maximum, so over the other 31/32 of
    // the rows the strip kernel only APPENDS the groups reaching tau_q (~31 k' per query) to a per-query candidate
    // list; one merge over {sample list} + {appended} gives exactly the k' groups the dense path selects. The Q x N/16
    // group-maximum matrix (2.56 GB at Q = 1024, N = 10M) is neither written nor read back. A query whose list overflows
    // (a tau_q far below the final one: sorted or clustered data) is handed to the widen pass by the guard.
    // It costs four extra small launches (~35 us), so it is taken when the matrix it avoids is worth more: from
    // Q x N = 10^9 scores (256 MB of group maxima written and read back). Option score_filter: 0 never, 2 whenever possible.
    p.nbn = p.Npad / 256;
    p.ns_tiles = std::max<int64_t>(16, p.nbn / std::max(1, mmiss_option("score_sample_div", 32)));
    const int filter_opt = mmiss_option("score_filter", 1);
    p.sample = p.big && p.nbn >= 128 && filter_opt != 0 && (filter_opt == 2 || (double)p.Mq * (double)p.Npad >= 1e9);
    p.Ndense = p.sample ? p.ns_tiles * 256 : p.Npad;   // rows whose group maxima are materialised
    if (p.big) p.strip = strip_length(p.Mq, p.nbn, p.sample ? p.nbn - p.ns_tiles : p.nbn, plan_options());
    if (p.sample) p.filter_cap = mmiss_option("score_filter_cap", 2048);
    return MMISS_OK;
}

// the query's predicate into ix->pend: its masks on the host and on the device (both null: an unfiltered query)
int stage_filter(mmiss_index* ix, hipStream_t st, int Q, const uint64_t* req, const uint64_t* exc) {
    mmiss_index::Pending& pd = ix->pend;
    pd.filt = req || exc;
    pd.d_mask = nullptr;
    if (!pd.filt) return MMISS_OK;
    if (req) MM_TRY(fetch_host(req, Q, pd.req, &st)); else pd.req.assign((size_t)Q, 0);
    if (exc) MM_TRY(fetch_host(exc, Q, pd.exc, &st)); else pd.exc.assign((size_t)Q, 0);
    MM_TRY(ix->fmask.ensure((size_t)Q * 16));
    MM_HIP(hipMemcpyAsync(ix->fmask.p, pd.req.data(), (size_t)Q * 8, hipMemcpyHostToDevice, st));
    MM_HIP(hipMemcpyAsync(ix->fmask.as<uint64_t>() + Q, pd.exc.data(), (size_t)Q * 8, hipMemcpyHostToDevice, st));
    pd.d_mask = ix->fmask.as<uint64_t>();
    return MMISS_OK;
}

// the query's result block into ix->pend: k slots per query and the guard's flags; device outputs without counts count into scratch
int stage_outputs(mmiss_index* ix, hipStream_t st, int Q, int k, bool out_dev, int64_t* out_labels, float* out_dist, int32_t* out_count) {
    mmiss_index::Pending& pd = ix->pend;
    pd.Q = Q; pd.k = k;
    MM_TRY(pd.out.stage(ix->pin, st, Q, k, out_dev, false, true, out_labels, out_dist, out_count, nullptr));
    if (!pd.out.cnt) {
        MM_TRY(ix->out_c.ensure((size_t)Q * 4));
        pd.out.cnt = ix->out_c.as<int32_t>();
    }
    return MMISS_OK;
}

// queries -> device, canonical normalisation: qn (f32, the re-rank's operand), qs (the first pass's operand) and eps_q (the
// guard's bound per query)
int upload_queries(mmiss_index* ix, hipStream_t st, const float* queries, int Q) {
    const int D = ix->dim;
    const int Qpad = (int)round_up(Q, 256);
    const float* qsrc = queries;
    MM_TRY(device_view(&qsrc, (size_t)Q * D, ix->qstage, 0, (size_t)Q * D * 4, st));
    MM_TRY(ix->qn.ensure((size_t)Qpad * D * 4));
    MM_TRY(ix->qs.ensure((size_t)Qpad * D * ix->qelt()));
    MM_TRY(ix->eps_q.ensure((size_t)Qpad * 4));
    MM_TRY(ix->thr.ensure((size_t)Qpad * 4));
    MM_PROF("prep_queries", st, 4.0 * Q * D, (double)Q * D * (8 + ix->elt));
    double eps_fixed, cnorm;
    guard_terms(ix, &eps_fixed, &cnorm);
    with_storage(ix->dtype, [&](auto s) {   // (f16 query operand for f16 and fp8 rows)
        using QT = typename decltype(s)::Q;
        hipLaunchKernelGGL(prep_queries_kernel<QT>, dim3((Qpad + 3) / 4), dim3(256), 0, st, qsrc, ix->qn.as<float>(), ix->qs.as<QT>(),
                           Q, Qpad, D, ix->eps_q.as<float>(), eps_fixed, cnorm);
    });
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// The dense first pass: the score GEMM writes the maximum of every group of 16 rows per query, select_topk / merge_lists keep
// the k' best groups per query as its candidates (threshold-filtered sample form: see plan_query).
int dense_pass(mmiss_index* ix, hipStream_t st, const QueryPlan& p, int Q) {
    const int D = ix->dim, kp = p.kp;
    const int64_t N = ix->count;
    // the pad rows up to the tile multiple are readable (capacity is a multiple of 1024) and masked in the epilogue
    const int ng = (int)(p.Ndense / 16);
    MM_TRY(ix->gmax.ensure((size_t)p.Mq * ng * 4));
    GemmEpi ep{};
    ep.out = ix->gmax.p; ep.ldo = ng; ep.m_valid = Q; ep.p0 = (int)N; ep.m_fast = 1;
    ep.aux = ix->inv.as<float>();   // (fp8 rows: inverse norms; null otherwise)
    {
        MM_PROF(p.dense8 ? (p.sample ? "score_gemm_f8_sample" : "score_gemm_f8") : (p.sample ? "score_gemm_f16_sample" : "score_gemm_f16"), st,
                2.0 * Q * (double)std::min<int64_t>(N, p.Ndense) * D, (double)std::min<int64_t>(N, p.Ndense) * D * ix->elt);
        if (p.big) MM_TRY(launch_strip_gemm(ix, st, p.strip_v3, ix->qs.p, ep, p.Mq, (int)p.Ndense, p.strip, nullptr));
        else MM_TRY((launch_gemm_inst<_Float16, 128, MMISS_EPI_GROUPMAX_F32>(st, ix->qs.p, ix->rows.p, ep, p.Mq, (int)p.Npad, D)));
    }
    const int splits = select_splits(ng, Q);
    MM_TRY(ix->lists_s.ensure((size_t)splits * Q * kp * 4));
    MM_TRY(ix->lists_r.ensure((size_t)splits * Q * kp * 4));
    SelectArgs sa{};
    sa.G = ix->gmax.as<float>(); sa.ldg = ng; sa.ng = ng; sa.kp = kp; sa.Q = Q;
    sa.out_s = ix->lists_s.as<float>(); sa.out_r = ix->lists_r.as<int32_t>();
    {
        MM_PROF("select_topk", st, 0.0, (double)Q * ng * 4);
        hipLaunchKernelGGL(select_topk_kernel, dim3(Q, splits), dim3(256), 0, st, sa);
        MM_HIP(hipGetLastError());
    }
    MergeArgs m{};
    m.in_s = ix->lists_s.as<float>(); m.in_r = ix->lists_r.as<int32_t>();
    m.L = splits; m.Q = Q; m.kp = kp;
    if (p.sample) {
        const int cap = p.filter_cap;
        MM_TRY(ix->seed_s.ensure((size_t)p.Mq * kp * 4));
        MM_TRY(ix->seed_r.ensure((size_t)p.Mq * kp * 4));
        MM_TRY(ix->fcnt.ensure((size_t)p.Mq * 4));
        MM_TRY(ix->fbuf_s.ensure((size_t)p.Mq * cap * 4));
        MM_TRY(ix->fbuf_g.ensure((size_t)p.Mq * cap * 4));
        {   // the sample's k' best groups per query WITH their scores: seed of the final merge, source of tau_q
            MergeArgs m1 = m;
            m1.lists_per_block = splits; m1.out_s = ix->seed_s.as<float>(); m1.out_r = ix->seed_r.as<int32_t>();
            MM_PROF("merge_lists", st, 0.0, (double)splits * Q * kp * 8);
            hipLaunchKernelGGL(merge_lists_kernel, dim3(Q, 1), dim3(256), 0, st, m1);
            MM_HIP(hipGetLastError());
        }
        MM_HIP(hipMemsetAsync(ix->fcnt.p, 0, (size_t)p.Mq * 4, st));
        StripFilter flt{};
        flt.tau = ix->seed_s.as<float>() + (kp - 1); flt.tau_stride = kp;
        flt.cnt = ix->fcnt.as<int32_t>(); flt.buf_s = ix->fbuf_s.as<float>(); flt.buf_g = ix->fbuf_g.as<int32_t>();
        flt.cap = cap; flt.bn_begin = (int)p.ns_tiles;
        {
            MM_PROF(p.dense8 ? "score_gemm_f8" : "score_gemm_f16", st, 2.0 * Q * (double)(N - p.Ndense) * D, (double)(N - p.Ndense) * D * ix->elt);
            MM_TRY(launch_strip_gemm(ix, st, p.strip_v3, ix->qs.p, ep, p.Mq, (int)p.Npad, p.strip, &flt));
        }
        m.in_s = ix->seed_s.as<float>(); m.in_r = ix->seed_r.as<int32_t>(); m.L = 1;
        m.flat_s = ix->fbuf_s.as<float>(); m.flat_r = ix->fbuf_g.as<int32_t>(); m.flat_cnt = ix->fcnt.as<int32_t>();
        m.flat_cap = cap;
    }
    m.cand = ix->cand.as<int32_t>(); m.cand_stride = p.ncand; m.page_off = 0;
    m.cur_s = ix->cur_s.as<float>(); m.cur_r = ix->cur_r.as<int32_t>();  // k'-th group maximum
    return launch_merge(ix, st, m);
}

// The paged streaming-scan first pass (filtered queries: its FILT form): per page, every slab's k' best rows per query, merged
// into the query's candidate page; a later page continues behind the last candidate of the one before (cur_s / cur_r).
int scan_pass(mmiss_index* ix, hipStream_t st, const QueryPlan& qp, int Q) {
    const mmiss_index::Pending& pd = ix->pend;
    const int kp = qp.kp;
    const ScanPlan p = plan_scan(ix->dim, ix->qelt(), Q, kp, ix->count, plan_options());
    MM_TRY(ix->lists_s.ensure((size_t)p.slabs * Q * kp * 4));
    MM_TRY(ix->lists_r.ensure((size_t)p.slabs * Q * kp * 4));
    const bool paging = qp.pages > 1;
    if (paging) {
        std::vector<float> inf((size_t)Q, INFINITY);
        std::vector<int32_t> neg((size_t)Q, -1);
        MM_HIP(hipMemcpyAsync(ix->cur_s.p, inf.data(), (size_t)Q * 4, hipMemcpyHostToDevice, st));
        MM_HIP(hipMemcpyAsync(ix->cur_r.p, neg.data(), (size_t)Q * 4, hipMemcpyHostToDevice, st));
        MM_HIP(hipStreamSynchronize(st));  // the host vectors go out of scope
    }
    for (int page = 0; page < qp.pages; ++page) {
        ScanArgs a{};
        a.rows = ix->rows.p; a.N = ix->count; a.D = ix->dim; a.inv = ix->inv.as<float>(); a.qs = ix->qs.p; a.Q = Q;
        a.cur_s = paging ? ix->cur_s.as<float>() : nullptr;
        a.cur_r = paging ? ix->cur_r.as<int32_t>() : nullptr;
        a.kp = kp; a.tiles_per_block = p.tiles_per_block;
        a.out_s = ix->lists_s.as<float>(); a.out_r = ix->lists_r.as<int32_t>();
        if (pd.filt) { a.tags = ix->tags.as<uint64_t>(); a.req = pd.d_mask; a.exc = pd.d_mask + Q; }
        MM_TRY(launch_scan(ix, st, a, p));
        MergeArgs m{};
        m.in_s = ix->lists_s.as<float>(); m.in_r = ix->lists_r.as<int32_t>();
        m.L = p.slabs; m.Q = Q; m.kp = kp;
        m.cand = ix->cand.as<int32_t>(); m.cand_stride = qp.ncand; m.page_off = page * kp;
        m.cur_s = ix->cur_s.as<float>(); m.cur_r = ix->cur_r.as<int32_t>();  // the scan reads them only when paging
        MM_TRY(launch_merge(ix, st, m));
    }
    return MMISS_OK;
}

// The first pass's canonical re-rank of the candidates: labels, distances and counts of ix->pend. With the guard on (see
// "exactness contract") it also writes a flag per query it cannot prove — one plain store per query into the pinned block,
// counted on the host — and the threshold the widen pass starts from.
int rerank_first(mmiss_index* ix, hipStream_t st, const QueryPlan& p) {
    const mmiss_index::Pending& pd = ix->pend;
    RerankArgs r{};
    r.rows = ix->rows.p; r.D = ix->dim; r.inv = ix->inv.as<float>(); r.qn = ix->qn.as<float>(); r.cand = ix->cand.as<int32_t>();
    r.cand_stride = p.ncand; r.ncand = p.dense ? p.ncand * 16 : p.ncand; r.group_mode = p.dense ? 1 : 0; r.nrows = ix->count;
    r.labels = ix->labels_d.as<int64_t>(); r.k = pd.k;
    r.out_labels = pd.out.lab; r.out_dist = pd.out.dist; r.out_count = pd.out.cnt;
    if (pd.guard) {
        r.tau = ix->cur_s.as<float>(); r.eps_q = ix->eps_q.as<float>();
        r.thr_out = ix->thr.as<float>();
        r.flags = pd.out.flags; r.nflag = nullptr;
        r.force_flag = mmiss_option("guard_force", 0);
        // threshold-filtered selection: per-query append counts and their capacity
        if (p.sample) { r.ovf_cnt = ix->fcnt.as<int32_t>(); r.ovf_cap = p.filter_cap; }
    }
    return launch_rerank(ix, st, r, pd.Q);
}

// Where a guarded query's widen pass goes (option query_side_stream, a diagnostic: the results are the same bits either way):
// 1 side_stream, 0 the handle's stream.
int side_stream_mode() { return mmiss_option("query_side_stream", 1); }

// first pass of a query: everything up to and including the rerank is QUEUED on the stream; ix->pend describes it
// req / exc: a filtered query's [Q] masks (host or device, null = 0; both null: unfiltered)
int query_begin_locked(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, const uint64_t* req, const uint64_t* exc,
                       int64_t* out_labels, float* out_dist, int32_t* out_count) {
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    const int64_t N = ix->count;
    mmiss_index::Pending& pd = ix->pend;
    bool out_dev = false;
    MM_TRY(outputs_all_host_or_all_device("mmiss_index_query", out_labels, out_dist, out_count, nullptr, &out_dev));
    MM_TRY(stage_filter(ix, st, Q, req, exc));
    MM_TRY(stage_outputs(ix, st, Q, k, out_dev, out_labels, out_dist, out_count));
    QueryPlan p;
    MM_TRY(plan_query(ix, Q, k, pd.filt, p));
    MM_TRY(upload_queries(ix, st, queries, Q));
    MM_TRY(ix->cand.ensure((size_t)Q * p.ncand * 4));
    // (score, row) of the last candidate stage 1 kept per query, -inf when it kept every row: the paging cursor, and the
    // guard's bound on what was left out
    MM_TRY(ix->cur_s.ensure((size_t)Q * 4));
    MM_TRY(ix->cur_r.ensure((size_t)Q * 4));
    if (N == 0) MM_HIP(hipMemsetAsync(ix->cand.p, 0xff, (size_t)Q * p.ncand * 4, st));  // all -1
    else if (p.dense) MM_TRY(dense_pass(ix, st, p, Q));
    else MM_TRY(scan_pass(ix, st, p, Q));
    pd.guard = N > 0 && mmiss_option("exact_guard", 1) != 0;
    MM_TRY(rerank_first(ix, st, p));
    ix->stat_queries += Q;
    MM_HIP(hipEventRecord(ix->done_ev, st));
    pd.active = true;
    return MMISS_OK;
}

// second half: wait for the first pass (its event, NOT the stream: the caller may have queued the next batch's encode behind
// it), widen what the guard could not prove, hand host outputs over.
// The widen pass runs on side_stream and needs NO edge: the host has seen done_ev, so everything it reads — qs, qn, thr, eps_q,
// the masks, the output rows the first re-rank wrote — is complete, and everything it writes is complete before this returns
// (sweep_queries drains the stream it is given), so whatever the caller queues afterwards sees it. On the caller's stream it
// would sit behind the work queued there since query_begin (the next batch's encode), and its waits would wait for that too.
int query_end_locked(mmiss_index* ix) {
    const mmiss_index::Pending& pd = ix->pend;   // (unchanged until the next query begins)
    ix->pend.active = false;
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    if (!pd.guard && pd.out.dev && ix->has_user_stream) {  // device outputs on the caller's stream, nothing to decide: stays queued
        ix->async_pending = true;
        return MMISS_OK;
    }
    MM_HIP(hipEventSynchronize(ix->done_ev));
    if (pd.guard) {
        std::vector<int32_t> which;
        for (int q = 0; q < pd.Q; ++q)
            if (pd.out.flags[q]) which.push_back(q);
        if (!which.empty()) {
            ix->stat_flagged += (int64_t)which.size();
            hipStream_t ws = side_stream_mode() != 0 ? ix->side_stream : st;
            const int rc = sweep_queries(ix, ws, pd, which);  // returns with `ws` drained
            if (rc != MMISS_OK) {
                // (the scratch buffers are the next call's, written by stream order on st: nothing may be left running beside it)
                if (ws != st) (void)hipStreamSynchronize(ws);
                return rc;
            }
        }
    }
    pd.out.deliver();
    return MMISS_OK;
}

// the four query entry points: req / exc the masks of a filtered query (both null: mmiss_index_query itself, same path, same
// results); begin_only leaves the query open for mmiss_index_query_end; `who` names the entry point in errors
int query_entry(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, const uint64_t* req, const uint64_t* exc,
                int64_t* out_labels, float* out_dist, int32_t* out_count, bool begin_only, const char* who) {
    if (!ix || !queries || !out_labels || !out_dist) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 0 || k <= 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d", who, Q, k);
    if (Q == 0) {
        if (begin_only) MM_FAIL(MMISS_ERR_ARG, "%s: Q = 0", who);
        return MMISS_OK;
    }
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    MM_TRY(query_begin_locked(ix, queries, Q, k, req, exc, out_labels, out_dist, out_count));
    return begin_only ? MMISS_OK : query_end_locked(ix);
}

}  // namespace

extern "C" int mmiss_index_query(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, int64_t* out_labels,
                                 float* out_dist, int32_t* out_count) {
    return query_entry(ix, queries, Q, k, nullptr, nullptr, out_labels, out_dist, out_count, false, "mmiss_index_query");
}

extern "C" int mmiss_index_query_begin(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, int64_t* out_labels,
                                       float* out_dist, int32_t* out_count) {
    return query_entry(ix, queries, Q, k, nullptr, nullptr, out_labels, out_dist, out_count, true, "mmiss_index_query_begin");
}

extern "C" int mmiss_index_query_filtered(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, const uint64_t* require,
                                          const uint64_t* exclude, int64_t* out_labels, float* out_dist, int32_t* out_count) {
    return query_entry(ix, queries, Q, k, require, exclude, out_labels, out_dist, out_count, false, "mmiss_index_query_filtered");
}

extern "C" int mmiss_index_query_filtered_begin(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, const uint64_t* require,
                                                const uint64_t* exclude, int64_t* out_labels, float* out_dist, int32_t* out_count) {
    return query_entry(ix, queries, Q, k, require, exclude, out_labels, out_dist, out_count, true, "mmiss_index_query_filtered_begin");
}

extern "C" int mmiss_index_query_end(mmiss_index* ix) {
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_query_end: null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->pend.active) MM_FAIL(MMISS_ERR_STATE, "mmiss_index_query_end: no query was begun");
    return query_end_locked(ix);
}

// Drop a query opened with mmiss_index_query_begin without taking its results: waits for the first pass that is queued (its
// kernels write the caller's output buffers and the handle's scratch), then frees the handle for other calls. A no-op when
// no query is open. Nothing can be in flight on side_stream then: a widen pass is queued only by query_end, which drains it.
extern "C" int mmiss_index_query_abort(mmiss_index* ix) {
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_query_abort: null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (!ix->pend.active) return MMISS_OK;
    ix->pend.active = false;
    MM_TRY(mmiss_use_device(ix->device));
    MM_HIP(hipEventSynchronize(ix->done_ev));
    return MMISS_OK;
}

extern "C" int mmiss_index_guard_stats_ex(mmiss_index* ix, int64_t out[8]) {
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_guard_stats_ex: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = ix->stat_queries; out[1] = ix->stat_flagged; out[2] = ix->stat_rounds; out[3] = ix->stat_pages;
    out[4] = ix->stat_exhaustive; out[5] = ix->stat_swept_rows;
    out[6] = ix->stat_radius_queries; out[7] = ix->stat_radius_pages;
    return MMISS_OK;
}

extern "C" int mmiss_index_guard_stats(mmiss_index* ix, int64_t out[4]) {
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_guard_stats: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    out[0] = ix->stat_queries; out[1] = ix->stat_flagged; out[2] = ix->stat_rounds; out[3] = ix->stat_pages;
    return MMISS_OK;
}

// ================================================================================================ radius queries
// "Every row at least this similar": the members of query q are the rows with a direction that q admits and whose canonical
// distance is <= max_dist[q] (float compare). It is the widen pass with the threshold taken from the caller's radius instead
// of a top-k's k-th score: ONE threshold pass (threshold_pass: thr_q = (1 - R) - eps_q, radius_thr_kernel has the derivation),
// the canonical re-rank with the cut (rerank_kernel<T, true>), and for a list of more than SWEEP_CAP rows the exhaustive
// canonical pass with a host selection. No first pass, no guard decision: a call costs one pass over the index per chunk on the
// score GEMM, one per 64 queries on the scan. Exact: ids and distance bits are the canonical arithmetic's.
namespace {

constexpr int RADIUS_CHUNK = 1024;   // queries per chunk: bounds the lists (SWEEP_CAP x 4 B each) and the pinned staging
constexpr int RADIUS_MAX_CAP = 4096;

// one radius call, as its chunks see it
struct RadiusCall {
    int cap = 0;
    const float* rad = nullptr;         // [Q] HOST radii (no NaN)
    const uint64_t* req = nullptr;      // [Q] masks as the caller passed them (host or device), null = 0
    const uint64_t* exc = nullptr;
    const int32_t* row_min = nullptr;   // [Q] HOST: later_only, the queries' own rows; null otherwise
    bool out_dev = false;
    int64_t* out_labels = nullptr; float* out_dist = nullptr; int32_t* out_count = nullptr; int64_t* out_total = nullptr;
};

// The exhaustive pass of a radius query: chunk query qc (radius R, masks of ix->pend, later_only: rows above row_min) against
// every row — the admitted rows with d <= R, all counted, the `cap` best by (distance, row) kept. `lab` / `dist`: [cap] host.
int radius_exhaustive(mmiss_index* ix, hipStream_t st, int32_t qc, float R, int64_t row_min, int cap, int64_t* lab, float* dist,
                      int32_t* count, int64_t* total) {
    const int64_t N = ix->count;
    const mmiss_index::Pending& pd = ix->pend;
    MM_TRY(ix->dist_all.ensure((size_t)N * 4));
    MM_TRY(ix->dist_pin.ensure((size_t)N * 4, st));
    MM_TRY(canonical_distances(ix, st, qc));
    const float* d_all = ix->dist_pin.as<float>();
    typedef std::pair<float, int32_t> Ent;  // (distance, row); NaN distances are no members (d <= R is false)
    std::vector<Ent> mem;
    const uint64_t rq = pd.filt ? pd.req[(size_t)qc] : 0, rx = pd.filt ? pd.exc[(size_t)qc] : 0;
    for (int64_t r = std::max<int64_t>(row_min + 1, 0); r < N; ++r) {
        const float d = d_all[(size_t)r];
        if (!(d <= R)) continue;
        if (pd.filt && !tag_admits_h(ix->tags_h[(size_t)r], rq, rx)) continue;
        mem.push_back(Ent(d, (int32_t)r));
    }
    const size_t keep = std::min<size_t>((size_t)cap, mem.size());
    std::partial_sort(mem.begin(), mem.begin() + keep, mem.end());
    for (int i = 0; i < cap; ++i) {
        lab[i] = (size_t)i < keep ? ix->labels_h[(size_t)mem[i].second] : -1;
        dist[i] = (size_t)i < keep ? mem[i].first : INFINITY;
    }
    *count = (int32_t)keep;
    *total = (int64_t)mem.size();
    ix->stat_exhaustive += 1;
    return MMISS_OK;
}

// One chunk of a radius call: queries [q0, q0 + Qc) of the call, `queries` pointing at the chunk's first (host or device).
// row_begin: no query of the chunk wants a row below it. Returns with the stream drained and the chunk's outputs delivered.
int radius_chunk(mmiss_index* ix, hipStream_t st, const RadiusCall& c, const float* queries, int64_t q0, int Qc, int64_t row_begin) {
    const int cap = c.cap;
    const int Qpad = (int)round_up(Qc, 256);
    MM_TRY(stage_filter(ix, st, Qc, c.req ? c.req + q0 : nullptr, c.exc ? c.exc + q0 : nullptr));
    const mmiss_index::Pending& pd = ix->pend;   // (the chunk's masks; no query is open: MM_NO_PENDING at the entry)
    ResultBlock out;   // with totals: the caller's, or scratch when device outputs come without them
    MM_TRY(out.stage(ix->pin, st, Qc, cap, c.out_dev, true, false, c.out_labels + q0 * cap, c.out_dist + q0 * cap, c.out_count + q0,
                     c.out_total ? c.out_total + q0 : nullptr));
    if (!out.tot) { MM_TRY(ix->rtotal.ensure((size_t)RADIUS_CHUNK * 8)); out.tot = ix->rtotal.as<int64_t>(); }
    MM_TRY(upload_queries(ix, st, queries, Qc));   // qn, qs (pad rows zero), eps_q
    MM_TRY(ix->rad.ensure((size_t)RADIUS_CHUNK * 4));
    MM_HIP(hipMemcpyAsync(ix->rad.p, c.rad + q0, (size_t)Qc * 4, hipMemcpyHostToDevice, st));
    if (c.row_min) {
        MM_TRY(ix->row_min.ensure((size_t)RADIUS_CHUNK * 4));
        MM_HIP(hipMemcpyAsync(ix->row_min.p, c.row_min + q0, (size_t)Qc * 4, hipMemcpyHostToDevice, st));
    }
    {
        MM_PROF("radius_thr", st, 2.0 * Qc, (double)Qpad * 12);
        hipLaunchKernelGGL(radius_thr_kernel, dim3((Qpad + 255) / 256), dim3(256), 0, st, ix->rad.as<float>(), ix->eps_q.as<float>(),
                           ix->thr.as<float>(), Qc, Qpad);
        MM_HIP(hipGetLastError());
    }
    int pages = 0;
    MM_TRY(threshold_pass(ix, st, Qc, ix->qs.p, ix->thr.as<float>(), pd.filt ? pd.d_mask : nullptr, row_begin, &pages));
    RerankArgs r{};
    r.k = cap;
    r.out_labels = out.lab; r.out_dist = out.dist; r.out_count = out.cnt; r.out_total = out.tot;
    r.max_dist = ix->rad.as<float>();
    r.row_min = c.row_min ? ix->row_min.as<int32_t>() : nullptr;
    std::vector<int32_t> over;
    MM_TRY(rerank_swept(ix, st, r, Qc, nullptr, true, over));
    MM_HIP(hipStreamSynchronize(st));
    ix->stat_radius_queries += Qc;
    ix->stat_radius_pages += pages;
    if (!over.empty()) {   // a list of more than SWEEP_CAP rows: one canonical pass and one host selection per such query
        std::vector<int64_t> xl((size_t)cap);
        std::vector<float> xd((size_t)cap);
        for (int32_t qc : over) {
            int32_t cnt = 0;
            int64_t tot = 0;
            MM_TRY(radius_exhaustive(ix, st, qc, c.rad[q0 + qc], c.row_min ? c.row_min[q0 + qc] : -1, cap, xl.data(), xd.data(), &cnt, &tot));
            if (c.out_dev) {
                MM_HIP(hipMemcpyAsync(out.lab + (size_t)qc * cap, xl.data(), (size_t)cap * 8, hipMemcpyHostToDevice, st));
                MM_HIP(hipMemcpyAsync(out.dist + (size_t)qc * cap, xd.data(), (size_t)cap * 4, hipMemcpyHostToDevice, st));
                MM_HIP(hipMemcpyAsync(out.cnt + qc, &cnt, 4, hipMemcpyHostToDevice, st));
                MM_HIP(hipMemcpyAsync(out.tot + qc, &tot, 8, hipMemcpyHostToDevice, st));
                MM_HIP(hipStreamSynchronize(st));   // (pageable sources, reused by the next query)
            } else {
                memcpy(out.lab + (size_t)qc * cap, xl.data(), (size_t)cap * 8);
                memcpy(out.dist + (size_t)qc * cap, xd.data(), (size_t)cap * 4);
                out.cnt[qc] = cnt;
                out.tot[qc] = tot;
            }
        }
    }
    out.deliver();
    return MMISS_OK;
}

// what the two entry points check alike; fills c's outputs and cap
int radius_check(const char* who, int cap, int64_t* out_labels, float* out_dist, int32_t* out_count, int64_t* out_total, RadiusCall& c) {
    if (!out_labels || !out_dist || !out_count) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (cap < 1 || cap > RADIUS_MAX_CAP) MM_FAIL(MMISS_ERR_ARG, "%s: cap = %d (1 .. %d result slots per query)", who, cap, RADIUS_MAX_CAP);
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_total, &c.out_dev));
    c.cap = cap;
    c.out_labels = out_labels; c.out_dist = out_dist; c.out_count = out_count; c.out_total = out_total;
    return MMISS_OK;
}

}  // namespace

extern "C" int mmiss_index_query_radius(mmiss_index* ix, const float* queries, int32_t Q, const float* max_dist, int32_t cap,
                                        const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                                        int32_t* out_count, int64_t* out_total) {
    const char* who = "mmiss_index_query_radius";
    if (!ix || (Q > 0 && (!queries || !max_dist))) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q = %d", who, Q);
    if (Q == 0) return MMISS_OK;
    RadiusCall c;
    MM_TRY(radius_check(who, cap, out_labels, out_dist, out_count, out_total, c));
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    std::vector<float> rad;
    MM_TRY(fetch_host(max_dist, Q, rad, &st));
    for (int q = 0; q < Q; ++q)
        if (rad[(size_t)q] != rad[(size_t)q]) MM_FAIL(MMISS_ERR_ARG, "%s: max_dist[%d] is NaN", who, q);
    c.rad = rad.data(); c.req = require; c.exc = exclude;
    for (int64_t q0 = 0; q0 < Q; q0 += RADIUS_CHUNK) {
        const int Qc = (int)std::min<int64_t>(RADIUS_CHUNK, Q - q0);
        MM_TRY(radius_chunk(ix, st, c, queries + q0 * ix->dim, q0, Qc, 0));
    }
    return MMISS_OK;
}

extern "C" int mmiss_index_query_radius_by_label(mmiss_index* ix, const int64_t* labels, int64_t n, float max_dist, int32_t cap,
                                                 int32_t later_only, int64_t* out_labels, float* out_dist, int32_t* out_count,
                                                 int64_t* out_total) {
    const char* who = "mmiss_index_query_radius_by_label";
    if (!ix || (n > 0 && !labels)) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (n < 0) MM_FAIL(MMISS_ERR_ARG, "%s: n = %lld", who, (long long)n);
    if (max_dist != max_dist) MM_FAIL(MMISS_ERR_ARG, "%s: max_dist is NaN", who);
    if (n == 0) return MMISS_OK;
    RadiusCall c;
    MM_TRY(radius_check(who, cap, out_labels, out_dist, out_count, out_total, c));
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    std::vector<int64_t> rows((size_t)n);
    std::vector<int32_t> rows32((size_t)n);
    for (int64_t i = 0; i < n; ++i) {   // every label first: a missing one writes nothing
        rows[(size_t)i] = find_row(ix, labels[i]);
        if (rows[(size_t)i] < 0) MM_FAIL(MMISS_ERR_ARG, "%s: label %lld not in the index", who, (long long)labels[i]);
        rows32[(size_t)i] = (int32_t)rows[(size_t)i];
    }
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    const std::vector<float> rad((size_t)n, max_dist);
    c.rad = rad.data();
    c.row_min = later_only ? rows32.data() : nullptr;
    const int D = ix->dim;
    for (int64_t q0 = 0; q0 < n; q0 += RADIUS_CHUNK) {
        const int Qc = (int)std::min<int64_t>(RADIUS_CHUNK, n - q0);
        // the chunk's queries: the rows the index represents, widened to f32 on the device (what mmiss_index_get returns)
        MM_TRY(ix->map.ensure((size_t)RADIUS_CHUNK * 8));
        MM_TRY(ix->stage.ensure((size_t)RADIUS_CHUNK * D * 4));
        MM_HIP(hipMemcpyAsync(ix->map.p, rows.data() + q0, (size_t)Qc * 8, hipMemcpyHostToDevice, st));
        {
            MM_PROF("rows_as_queries", st, 0.0, (double)Qc * D * (4 + ix->elt));
            const int grid = (int)std::min<int64_t>(4096, ((int64_t)Qc * D + 255) / 256);
            with_storage(ix->dtype, [&](auto s) {
                using T = typename decltype(s)::T;
                hipLaunchKernelGGL(rows_as_queries_kernel<T>, dim3(grid), dim3(256), 0, st, ix->rows.as<T>(), (const float*)ix->inv.as<float>(),
                                   ix->map.as<int64_t>(), ix->stage.as<float>(), (int64_t)Qc, D);
            });
            MM_HIP(hipGetLastError());
        }
        // later_only: a query wants rows above its own only, so the pass may start at the chunk's smallest row
        int64_t row_begin = 0;
        if (later_only) row_begin = *std::min_element(rows.begin() + q0, rows.begin() + q0 + Qc);
        MM_TRY(radius_chunk(ix, st, c, ix->stage.as<float>(), q0, Qc, row_begin));
    }
    return MMISS_OK;
}

// ================================================================================================ membership / tagging
// The DENSE form of the radius question: for P <= 64 probes (a query vector and a radius each) the exact membership of every row,
// one bit per (row, probe) — the member definition of mmiss_index_query_radius, with no cap on the members, because the answer
// is a bit per row and not a list. membership_kernels.h has the kernels and the two-sided bound; the three routes:
//   scan      member_scan_kernel decides every pair whose approximate score clears hi_p = (1 - R_p) + eps_p (member) or stays
//             below lo_p = (1 - R_p) - eps_p (no member); one pass over the index per 16 * nqt probes;
//   resolve   the borderline pairs in between, listed per probe (ix->swp_cnt / ix->swp_list, SWEEP_CAP rows per probe), get their
//             canonical distance (member_resolve_kernel);
//   overflow  a probe with more than SWEEP_CAP borderline rows: canonical_scan_kernel + member_from_dist_kernel, on the device
//             (radius_exhaustive's host selection has nothing to select here).
namespace {

// One dense scan of every row (plan_dense, by passes) by a kernel family K — K::kernel<T, NQT>() over K::Args —: the instantiation
// for the index's rows and the plan's operand tile, its dynamic LDS, and one launch per pass of 16 * nqt operands. The arguments
// every family shares are set here; fill(a, j, NQ) adds pass j's own. prof: the family's profile names for f32 / f16 / fp8 rows;
// state_bytes: what a pass moves per row beside the row.
template <typename K, typename Fill>
int launch_dense_scan(mmiss_index* ix, hipStream_t st, const DensePlan& p, const char* const (&prof)[3], int state_bytes, Fill&& fill) {
    typedef typename K::Args Args;
    typedef void (*Kern)(Args);
    const Kern kern = with_storage(ix->dtype, [&](auto s) -> Kern {
        using T = typename decltype(s)::T;
        if (p.nqt == 4) return K::template kernel<T, 4>();
        if (p.nqt == 2) return K::template kernel<T, 2>();
        return K::template kernel<T, 1>();
    });
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), p.lds));
    const int NQ = 16 * p.nqt, D = ix->dim;
    const int64_t N = ix->count;
    const char* const name = prof[ix->dtype == MMISS_F16 ? 1 : ix->dtype == MMISS_F8 ? 2 : 0];
    for (int j = 0; j < p.passes; ++j) {
        Args a{};
        a.rows = ix->rows.p; a.N = N; a.D = D; a.inv = ix->inv.as<float>();
        a.qs = ix->qs.as<char>() + (size_t)j * NQ * D * ix->qelt();
        a.tiles_per_block = p.tiles_per_block;
        fill(a, j, NQ);
        MM_PROF(name, st, 2.0 * NQ * (double)N * D, (double)N * (D * ix->elt + state_bytes));
        hipLaunchKernelGGL(kern, dim3(p.slabs), dim3(256), p.lds, st, a);
        MM_HIP(hipGetLastError());
    }
    return MMISS_OK;
}

struct MemberScan {
    typedef MemberScanArgs Args;
    template <typename T, int NQT> static auto kernel() { return &member_scan_kernel<T, NQT>; }
};

// Bit p of d_words[r] (device, [count]) = row r is a member of probe p, bits >= P zero. rad: [P] HOST radii (no NaN), left on
// the device in ix->mem_thr ([64] floats). count > 0. Waits once, for the lists' lengths (launching the resolve blind, with a
// fixed grid, and delivering before the lengths are known saved nothing measurable: profiles/membership.txt); what it queues
// behind that wait is left to the caller's final synchronisation.
int membership_core(mmiss_index* ix, hipStream_t st, const float* queries, int P, const float* rad, uint64_t* d_words) {
    const int D = ix->dim;
    const int64_t N = ix->count;
    MM_TRY(upload_queries(ix, st, queries, P));   // qn, qs (rows behind P zero, 256 of them at least), eps_q
    MM_TRY(ix->mem_thr.ensure((size_t)4 * 64 * 4));
    float* const d_rad = ix->mem_thr.as<float>();
    float* const d_lo = d_rad + 64;
    float* const d_hi = d_rad + 128;
    MM_HIP(hipMemcpyAsync(d_rad, rad, (size_t)P * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(member_thr_kernel, dim3(1), dim3(64), 0, st, (const float*)d_rad, (const float*)ix->eps_q.as<float>(), d_lo, d_hi, P, 64);
    MM_HIP(hipGetLastError());
    const size_t cnt_bytes = (size_t)64 * MEMBER_CNT_STRIDE * 4;   // one counter per probe, 256 bytes apart
    MM_TRY(ix->swp_cnt.ensure(cnt_bytes));
    MM_TRY(ix->swp_list.ensure((size_t)64 * SWEEP_CAP * 4));
    MM_TRY(ix->swp_pin.ensure(cnt_bytes, st));
    MM_HIP(hipMemsetAsync(ix->swp_cnt.p, 0, cnt_bytes, st));
    const DensePlan mp = plan_dense(D, ix->qelt(), P, N, true);
    if (mp.lds > SCAN_LDS_LIMIT)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "membership: a 16-probe block of dim %d does not fit the LDS (%d bytes)", D, mp.lds);
    MM_TRY(launch_dense_scan<MemberScan>(ix, st, mp, {"member_scan_f32", "member_scan_f16", "member_scan_f8"}, 8, [&](MemberScanArgs& a, int j, int NQ) {
        a.lo = d_lo + j * NQ; a.hi = d_hi + j * NQ;
        a.words = d_words; a.bit0 = j * NQ; a.first = j == 0;
        a.bcnt = ix->swp_cnt.as<int32_t>() + (size_t)j * NQ * MEMBER_CNT_STRIDE;
        a.blist = ix->swp_list.as<int32_t>() + (size_t)j * NQ * SWEEP_CAP;
        a.bcap = SWEEP_CAP;
    }));
    // the lists' lengths decide the rest
    MM_HIP(hipMemcpyAsync(ix->swp_pin.p, ix->swp_cnt.p, cnt_bytes, hipMemcpyDeviceToHost, st));
    MM_HIP(hipStreamSynchronize(st));
    const int32_t* cnt = ix->swp_pin.as<int32_t>();   // (one per probe, MEMBER_CNT_STRIDE apart)
    std::vector<int> over;
    int64_t resolved = 0;
    int maxc = 0;
    for (int p = 0; p < P; ++p) {
        const int32_t c = cnt[p * MEMBER_CNT_STRIDE];
        if (c > SWEEP_CAP) over.push_back(p);
        else { resolved += c; maxc = std::max(maxc, (int)c); }
    }
    if (maxc > 0) {
        MM_PROF("member_resolve", st, 2.0 * resolved * D, (double)resolved * D * ix->elt);
        const int grid = std::min(512, (maxc + 15) / 16);
        with_storage(ix->dtype, [&](auto s) {
            using T = typename decltype(s)::T;
            hipLaunchKernelGGL(member_resolve_kernel<T>, dim3(grid, P), dim3(256), 0, st, (const void*)ix->rows.p, D, (const float*)ix->qn.as<float>(),
                               (const float*)ix->inv.as<float>(), (const float*)d_rad, (const int32_t*)ix->swp_cnt.as<int32_t>(),
                               (const int32_t*)ix->swp_list.as<int32_t>(), SWEEP_CAP, d_words);
        });
        MM_HIP(hipGetLastError());
    }
    for (int p : over) {   // more than SWEEP_CAP rows within eps of the probe's threshold: every row's canonical distance decides
        MM_TRY(ix->dist_all.ensure((size_t)N * 4));
        MM_TRY(launch_canonical_scan(ix, st, p));
        hipLaunchKernelGGL(member_from_dist_kernel, dim3(member_from_dist_grid(N)), dim3(256), 0, st,
                           (const float*)ix->dist_all.as<float>(), N, (const float*)d_rad, p, d_words);
        MM_HIP(hipGetLastError());
    }
    ix->stat_radius_queries += P;
    ix->stat_radius_pages += mp.passes;
    ix->stat_swept_rows += resolved + (int64_t)over.size() * N;
    ix->stat_exhaustive += (int64_t)over.size();
    return MMISS_OK;
}

// the members of every probe, counted from the words into ix->mem_cnt ([64] u64)
int membership_counts(mmiss_index* ix, hipStream_t st, const uint64_t* d_words) {
    MM_TRY(ix->mem_cnt.ensure((size_t)64 * 8));
    MM_HIP(hipMemsetAsync(ix->mem_cnt.p, 0, (size_t)64 * 8, st));
    hipLaunchKernelGGL(member_count_kernel, dim3(member_count_grid(ix->count)), dim3(256), 0, st, d_words, ix->count,
                       ix->mem_cnt.as<unsigned long long>());
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// out_members (host or device, may be null) <- the first P counts of ix->mem_cnt, or zeros (an empty index)
int deliver_members(mmiss_index* ix, hipStream_t st, int P, int64_t* out_members, bool zeros) {
    if (!out_members) return MMISS_OK;
    if (zeros) return zero_any(out_members, (size_t)P * 8, st, true);
    return copy_any(out_members, ix->mem_cnt.p, (size_t)P * 8, st);
}

// what both entry points check before they touch anything; on success `rad` holds the P radii on the host
int membership_check(mmiss_index* ix, const char* who, int32_t P, const float* max_dist, hipStream_t* st, std::vector<float>& rad) {
    MM_TRY(enter(ix, who, st));
    MM_TRY(fetch_host(max_dist, P, rad, st));
    for (int p = 0; p < P; ++p)
        if (rad[(size_t)p] != rad[(size_t)p]) MM_FAIL(MMISS_ERR_ARG, "%s: max_dist[%d] is NaN", who, p);
    return MMISS_OK;
}

}  // namespace

extern "C" int mmiss_index_membership(mmiss_index* ix, const float* queries, int32_t P, const float* max_dist, uint64_t* out_words,
                                      int64_t cap_rows, int64_t* out_members) {
    const char* who = "mmiss_index_membership";
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "%s: null index", who);
    if (P < 1 || P > 64) MM_FAIL(MMISS_ERR_ARG, "%s: P = %d (1 .. 64 probes per call)", who, P);
    if (!queries || !max_dist) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (cap_rows < ix->count) MM_FAIL(MMISS_ERR_ARG, "%s: cap_rows = %lld for %lld rows", who, (long long)cap_rows, (long long)ix->count);
    if (ix->count > 0 && !out_words) MM_FAIL(MMISS_ERR_ARG, "%s: null out_words", who);
    hipStream_t st = nullptr;
    std::vector<float> rad;
    MM_TRY(membership_check(ix, who, P, max_dist, &st, rad));
    const int64_t N = ix->count;
    if (N == 0) {   // nothing to write but the counts
        ix->stat_radius_queries += P;
        return deliver_members(ix, st, P, out_members, true);
    }
    const bool out_dev = mmiss_is_device_ptr(out_words);
    uint64_t* d_words = out_words;
    if (!out_dev) { MM_TRY(ix->mem_words.ensure((size_t)N * 8)); d_words = ix->mem_words.as<uint64_t>(); }
    MM_TRY(membership_core(ix, st, queries, P, rad.data(), d_words));
    if (out_members) MM_TRY(membership_counts(ix, st, d_words));
    if (!out_dev) MM_TRY(copy_any(out_words, d_words, (size_t)N * 8, st));
    MM_TRY(deliver_members(ix, st, P, out_members, false));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

extern "C" int mmiss_index_tag_by_radius(mmiss_index* ix, const float* queries, int32_t P, const float* max_dist, const int32_t* bits,
                                         int64_t* out_members) {
    const char* who = "mmiss_index_tag_by_radius";
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "%s: null index", who);
    if (P < 1 || P > 64) MM_FAIL(MMISS_ERR_ARG, "%s: P = %d (1 .. 64 probes per call)", who, P);
    if (!queries || !max_dist || !bits) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    uint64_t mask = 0;
    for (int p = 0; p < P; ++p) {
        if (bits[p] < 0 || bits[p] > 63) MM_FAIL(MMISS_ERR_ARG, "%s: bits[%d] = %d (0 .. 63)", who, p, bits[p]);
        if (mask & (1ull << bits[p])) MM_FAIL(MMISS_ERR_ARG, "%s: bit %d is named twice", who, bits[p]);
        mask |= 1ull << bits[p];
    }
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    std::vector<float> rad;
    MM_TRY(membership_check(ix, who, P, max_dist, &st, rad));
    const int64_t N = ix->count;
    if (N == 0) {
        ix->stat_radius_queries += P;
        return deliver_members(ix, st, P, out_members, true);
    }
    MM_TRY(ix->mem_words.ensure((size_t)N * 8));
    uint64_t* const d_words = ix->mem_words.as<uint64_t>();
    MM_TRY(membership_core(ix, st, queries, P, rad.data(), d_words));
    if (out_members) MM_TRY(membership_counts(ix, st, d_words));
    // the merge under the named bits, then the host mirror (get_tags, remove and the exhaustive passes read it)
    int32_t* const d_bits = reinterpret_cast<int32_t*>(ix->mem_thr.as<float>() + 192);
    MM_HIP(hipMemcpyAsync(d_bits, bits, (size_t)P * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(member_merge_tags_kernel, dim3(member_merge_tags_grid(N)), dim3(256), 0, st, ix->tags.as<uint64_t>(),
                       (const uint64_t*)d_words, N, (const int32_t*)d_bits, P, mask);
    MM_HIP(hipGetLastError());
    MM_HIP(hipMemcpyAsync(ix->tags_h.data(), ix->tags.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    MM_TRY(deliver_members(ix, st, P, out_members, false));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// ================================================================================================ assignment / clustering
// The transposed question of a query: for EVERY row, which of C <= 1024 centres is nearest (canonical distance, ties to the
// smaller centre index) — zero-shot classification of the collection, the assignment step of spherical k-means — and the
// reduction its update step needs: the sums of the rows of every cluster, in a fixed-point form that has one value whatever
// order the hardware adds in. assign_kernels.h has the kernels and the proof of the sure / borderline split.
namespace {

constexpr int ASSIGN_MAX_CENTRES = 1024;
constexpr size_t ASSIGN_META_SIZES = 64;   // byte offset of the [1024] u64 sizes in asg_meta; in front: float E, int live, int borderline

// sizes of clusters [0, C) of d_assign (device, [count]) -> out_sizes (host or device); queued, not waited for
int assign_sizes(mmiss_index* ix, hipStream_t st, const int32_t* d_assign, int C, int64_t* out_sizes) {
    unsigned long long* const d_sizes = reinterpret_cast<unsigned long long*>(ix->asg_meta.as<char>() + ASSIGN_META_SIZES);
    MM_HIP(hipMemsetAsync(d_sizes, 0, (size_t)C * 8, st));
    hipLaunchKernelGGL(assign_sizes_kernel, dim3(assign_sizes_grid(ix->count)), dim3(256), 0, st, d_assign, ix->count, C, d_sizes);
    MM_HIP(hipGetLastError());
    return copy_any(out_sizes, d_sizes, (size_t)C * 8, st);
}

struct AssignScan {
    typedef AssignScanArgs Args;
    template <typename T, int NQT> static auto kernel() { return &assign_scan_kernel<T, NQT>; }
};

}  // namespace

extern "C" int mmiss_index_assign(mmiss_index* ix, const float* centres, int32_t C, int32_t* out_assign, float* out_dist, int64_t cap_rows,
                                  int64_t* out_sizes) {
    const char* who = "mmiss_index_assign";
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "%s: null index", who);
    if (C < 1 || C > ASSIGN_MAX_CENTRES) MM_FAIL(MMISS_ERR_ARG, "%s: C = %d (1 .. %d centres per call)", who, C, ASSIGN_MAX_CENTRES);
    if (!centres) MM_FAIL(MMISS_ERR_ARG, "%s: null centres", who);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (cap_rows < ix->count) MM_FAIL(MMISS_ERR_ARG, "%s: cap_rows = %lld for %lld rows", who, (long long)cap_rows, (long long)ix->count);
    if (ix->count > 0 && !out_assign) MM_FAIL(MMISS_ERR_ARG, "%s: null out_assign", who);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    const int64_t N = ix->count;
    const int D = ix->dim;
    if (N == 0) {   // nothing to write but the sizes
        ix->stat_radius_queries += C;
        return zero_any(out_sizes, (size_t)C * 8, st, true);
    }
    const DensePlan mp = plan_dense(D, ix->qelt(), C, N, true);   // the centre tile and the slabs: §4c's choice
    if (mp.lds > SCAN_LDS_LIMIT)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: a 16-centre block of dim %d does not fit the LDS (%d bytes)", who, D, mp.lds);
    const bool asg_dev = mmiss_is_device_ptr(out_assign), dist_dev = out_dist && mmiss_is_device_ptr(out_dist);
    MM_TRY(ix->asg_out.ensure((size_t)N * 8));
    MM_TRY(ix->asg_state.ensure((size_t)N * 12));
    MM_TRY(ix->asg_list.ensure((size_t)N * 4));
    MM_TRY(ix->asg_meta.ensure(ASSIGN_META_SIZES + (size_t)ASSIGN_MAX_CENTRES * 8));
    MM_TRY(ix->swp_pin.ensure(16, st));
    int32_t* const d_assign = asg_dev ? out_assign : ix->asg_out.as<int32_t>();
    float* const d_dist = !out_dist ? nullptr : dist_dev ? out_dist : ix->asg_out.as<float>() + N;
    float* const st_s1 = ix->asg_state.as<float>();
    int32_t* const st_i1 = reinterpret_cast<int32_t*>(st_s1 + N);
    float* const st_s2 = st_s1 + 2 * N;
    float* const d_E = ix->asg_meta.as<float>();
    int32_t* const d_live = ix->asg_meta.as<int32_t>() + 1;
    int32_t* const d_bcnt = ix->asg_meta.as<int32_t>() + 2;
    MM_TRY(upload_queries(ix, st, centres, C));   // qn, qs (rows behind C zero, 256 of them at least), eps_q
    const float* const eps = ix->eps_q.as<float>();
    MM_HIP(hipMemsetAsync(d_bcnt, 0, 4, st));
    hipLaunchKernelGGL(assign_bound_kernel, dim3(1), dim3(64), 0, st, eps, (int)C, d_E, d_live);
    MM_HIP(hipGetLastError());
    MM_TRY(launch_dense_scan<AssignScan>(ix, st, mp, {"assign_scan_f32", "assign_scan_f16", "assign_scan_f8"}, 12, [&](AssignScanArgs& a, int j, int NQ) {
        a.eps_q = eps;
        a.c0 = j * NQ; a.C = C; a.first = j == 0;
        a.st_s1 = st_s1; a.st_i1 = st_i1; a.st_s2 = st_s2;
    }));
    hipLaunchKernelGGL(assign_decide_kernel, dim3(assign_decide_grid(N)), dim3(256), 0, st, (const float*)st_s1,
                       (const int32_t*)st_i1, (const float*)st_s2, N, (const float*)d_E, d_assign, d_dist, ix->asg_list.as<int32_t>(), d_bcnt);
    MM_HIP(hipGetLastError());
    // the resolve kernels are launched blind: the list's length stays on the device
    const int rgrid = assign_resolve_grid(N);
    with_storage(ix->dtype, [&](auto s) {
        using T = typename decltype(s)::T;
        if (d_dist) {   // the sure rows' one distance
            MM_PROF("assign_dist", st, 2.0 * N * D, (double)N * D * ix->elt);
            hipLaunchKernelGGL(assign_resolve_kernel<T>, dim3(rgrid), dim3(256), 0, st, (const void*)ix->rows.p, D, (const float*)ix->qn.as<float>(),
                               (const float*)ix->inv.as<float>(), eps, (int)C, (const int32_t*)nullptr, (const int32_t*)nullptr, N, d_assign, d_dist);
        }
        MM_PROF("assign_resolve", st, 0.0, 0.0);
        hipLaunchKernelGGL(assign_resolve_kernel<T>, dim3(rgrid), dim3(256), 0, st, (const void*)ix->rows.p, D, (const float*)ix->qn.as<float>(),
                           (const float*)ix->inv.as<float>(), eps, (int)C, (const int32_t*)ix->asg_list.as<int32_t>(), (const int32_t*)d_bcnt, N,
                           d_assign, d_dist);
    });
    MM_HIP(hipGetLastError());
    if (out_sizes) MM_TRY(assign_sizes(ix, st, d_assign, C, out_sizes));
    if (!asg_dev) MM_TRY(copy_any(out_assign, d_assign, (size_t)N * 4, st));
    if (out_dist && !dist_dev) MM_TRY(copy_any(out_dist, d_dist, (size_t)N * 4, st));
    MM_HIP(hipMemcpyAsync(ix->swp_pin.p, ix->asg_meta.p, 12, hipMemcpyDeviceToHost, st));
    MM_HIP(hipStreamSynchronize(st));
    const int32_t* meta = ix->swp_pin.as<int32_t>();   // (E, live centres, borderline rows)
    ix->stat_radius_queries += C;
    ix->stat_radius_pages += mp.passes;
    ix->stat_swept_rows += (int64_t)meta[2] * meta[1];
    return MMISS_OK;
}

extern "C" int mmiss_index_cluster_sums(mmiss_index* ix, const int32_t* assign, int64_t n, int32_t C, int64_t* out_sums, int64_t* out_sizes) {
    const char* who = "mmiss_index_cluster_sums";
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "%s: null index", who);
    if (C < 1 || C > ASSIGN_MAX_CENTRES) MM_FAIL(MMISS_ERR_ARG, "%s: C = %d (1 .. %d clusters per call)", who, C, ASSIGN_MAX_CENTRES);
    if (!out_sums || (n > 0 && !assign)) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    std::lock_guard<std::mutex> lk(ix->mu);
    if (n != ix->count) MM_FAIL(MMISS_ERR_ARG, "%s: %lld assignments for %lld rows", who, (long long)n, (long long)ix->count);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    const int64_t N = ix->count;
    const int D = ix->dim;
    const size_t sum_bytes = (size_t)C * D * 8;
    if (N == 0) {
        MM_TRY(zero_any(out_sums, sum_bytes, st, false));
        MM_TRY(zero_any(out_sizes, (size_t)C * 8, st, true));
        MM_HIP(hipStreamSynchronize(st));
        return MMISS_OK;
    }
    MM_TRY(ix->asg_meta.ensure(ASSIGN_META_SIZES + (size_t)ASSIGN_MAX_CENTRES * 8));
    const int32_t* d_assign = assign;
    MM_TRY(device_view(&d_assign, (size_t)N, ix->asg_out, 0, (size_t)N * 4, st));
    const bool sums_dev = mmiss_is_device_ptr(out_sums);
    unsigned long long* d_sums = reinterpret_cast<unsigned long long*>(out_sums);
    if (!sums_dev) { MM_TRY(ix->asg_sums.ensure(sum_bytes)); d_sums = ix->asg_sums.as<unsigned long long>(); }
    MM_HIP(hipMemsetAsync(d_sums, 0, sum_bytes, st));
    const ClusterSumsPlan cp = plan_cluster_sums(D, C, N);
    ClusterSumsArgs a{};
    a.cols = cp.cols; a.rows_per_block = cp.rows_per_block;
    a.rows = ix->rows.p; a.inv = ix->inv.as<float>(); a.assign = d_assign; a.N = N; a.D = D; a.C = C; a.sums = d_sums;
    {
        MM_PROF("cluster_sums", st, (double)N * D, (double)N * (D * ix->elt + 4));
        int rc = MMISS_OK;
        with_storage(ix->dtype, [&](auto s) {
            using T = typename decltype(s)::T;
            rc = mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&cluster_sums_kernel<T>), cp.lds);
            if (rc == MMISS_OK) hipLaunchKernelGGL(cluster_sums_kernel<T>, dim3(cp.slabs, cp.chunks), dim3(1024), cp.lds, st, a);
        });
        MM_TRY(rc);
        MM_HIP(hipGetLastError());
    }
    if (out_sizes) MM_TRY(assign_sizes(ix, st, d_assign, C, out_sizes));
    if (!sums_dev) MM_TRY(copy_any(out_sums, d_sums, sum_bytes, st));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// ================================================================================================ partitioned search
// An inverted-file search on the centres and cells the assignment calls produce: a query reads only the rows of the nprobe cells
// whose centres are nearest to it, and the rows added since the partition was set. The approximation is in WHICH rows are looked
// at — that set is defined exactly (partition_kernels.h) —; within it the answer is the exact top-k with mmiss_index_query's
// distance bits and order, so probing every cell returns mmiss_index_query's bits. No first pass, no guard: every candidate gets
// its canonical distance, and the eight guard counters stay as they are.
namespace {

constexpr int PROBE_MAX_K = 2040;   // the flat query's own limit

// how a probed call of Q queries runs on the partition as it stands and under the options as they stand (index_plans.h)
ProbePlan plan_probed(const mmiss_index* ix, int Q, int k, int nprobe) {
    const mmiss_index::Partition& pt = ix->part;
    return plan_probed(ix->count, pt.B, pt.largest, pt.top_prefix.data(), pt.C, Q, k, nprobe, plan_options());
}

// what the partition calls check alike
#define MM_NEED_PARTITION(ix, who) \
    do { if ((ix)->part.C == 0) MM_FAIL(MMISS_ERR_STATE, "%s: the index has no partition (mmiss_index_partition_set)", who); } while (0)

}  // namespace

extern "C" int mmiss_index_partition_set(mmiss_index* ix, const float* centres, int32_t C, const int32_t* cells, int64_t n) {
    const char* who = "mmiss_index_partition_set";
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "%s: null index", who);
    if (C < 1 || C > PROBE_MAX_CENTRES) MM_FAIL(MMISS_ERR_ARG, "%s: C = %d (1 .. %d centres)", who, C, PROBE_MAX_CENTRES);
    if (!centres || n < 0 || (n > 0 && !cells)) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    if (n != ix->count) MM_FAIL(MMISS_ERR_ARG, "%s: %lld cells for %lld rows", who, (long long)n, (long long)ix->count);
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    const int D = ix->dim;
    // everything is built into fresh buffers and swapped in at the end: a refused call keeps the previous partition
    mmiss_index::Partition fresh;
    MM_TRY(fresh.cn.alloc((size_t)C * D * 4));
    MM_TRY(fresh.cells.alloc((size_t)std::max<int64_t>(n, 1) * 4));
    MM_TRY(fresh.off.alloc((size_t)(C + 1) * 4));
    // the small block: live [1024] int32, sizes [1024] u64, cursors [1024] int32
    MM_TRY(ix->prb_meta.ensure((size_t)PROBE_MAX_CENTRES * 16));
    int32_t* const d_live = ix->prb_meta.as<int32_t>();
    unsigned long long* const d_sizes = reinterpret_cast<unsigned long long*>(ix->prb_meta.as<char>() + (size_t)PROBE_MAX_CENTRES * 4);
    int32_t* const d_cursor = reinterpret_cast<int32_t*>(ix->prb_meta.as<char>() + (size_t)PROBE_MAX_CENTRES * 12);
    const float* src = centres;
    MM_TRY(device_view(&src, (size_t)C * D, ix->stage, 0, (size_t)C * D * 4, st));
    {   // the canonical normalisation of an f32 row: what oracle normalize_rows(centres, "f32") restates
        MM_PROF("normalize_rows", st, 4.0 * C * D, 8.0 * C * D);
        hipLaunchKernelGGL(normalize_rows_kernel<float>, dim3((C + 3) / 4), dim3(256), 0, st, src, fresh.cn.as<float>(), (int64_t)C, D);
        MM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(partition_live_kernel, dim3((C + 3) / 4), dim3(256), 0, st, (const float*)fresh.cn.as<float>(), (int)C, D, d_live);
    MM_HIP(hipGetLastError());
    MM_TRY(copy_any(fresh.cells.p, cells, (size_t)n * 4, st));
    MM_HIP(hipMemsetAsync(d_sizes, 0, (size_t)C * 8, st));
    if (n > 0) {
        hipLaunchKernelGGL(assign_sizes_kernel, dim3(assign_sizes_grid(n)), dim3(256), 0, st,
                           (const int32_t*)fresh.cells.as<int32_t>(), n, (int)C, d_sizes);
        MM_HIP(hipGetLastError());
    }
    std::vector<int32_t> live((size_t)C);
    std::vector<unsigned long long> sizes((size_t)C);
    MM_HIP(hipMemcpyAsync(live.data(), d_live, (size_t)C * 4, hipMemcpyDeviceToHost, st));
    MM_HIP(hipMemcpyAsync(sizes.data(), d_sizes, (size_t)C * 8, hipMemcpyDeviceToHost, st));
    MM_HIP(hipStreamSynchronize(st));
    if (std::find(live.begin(), live.end(), 1) == live.end())
        MM_FAIL(MMISS_ERR_ARG, "%s: none of the %d centres has a direction; the previous partition is kept", who, C);
    // the counting sort: offsets = the prefix of the sizes, then the scatter
    std::vector<int32_t> off((size_t)C + 1, 0);
    fresh.C = C; fresh.B = n;
    fresh.sizes.resize((size_t)C);
    for (int c = 0; c < C; ++c) {
        const int64_t sz = (int64_t)sizes[(size_t)c];
        fresh.sizes[(size_t)c] = sz;
        off[(size_t)c + 1] = off[(size_t)c] + (int32_t)sz;
        fresh.largest = std::max(fresh.largest, sz);
        fresh.empty += sz == 0;
    }
    fresh.in_cells = off[(size_t)C];
    std::vector<int64_t> desc(fresh.sizes);
    std::sort(desc.begin(), desc.end(), std::greater<int64_t>());
    fresh.top_prefix.assign((size_t)C + 1, 0);
    for (int c = 0; c < C; ++c) fresh.top_prefix[(size_t)c + 1] = fresh.top_prefix[(size_t)c] + desc[(size_t)c];
    MM_TRY(fresh.order.alloc((size_t)std::max<int64_t>(fresh.in_cells, 1) * 4));
    MM_HIP(hipMemcpyAsync(fresh.off.p, off.data(), (size_t)(C + 1) * 4, hipMemcpyHostToDevice, st));
    MM_HIP(hipMemcpyAsync(d_cursor, off.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
    if (n > 0) {
        MM_PROF("partition_fill", st, 0.0, 8.0 * n);
        hipLaunchKernelGGL(partition_fill_kernel, dim3((int)((n + PART_FILL_ROWS - 1) / PART_FILL_ROWS)), dim3(256), 0, st,
                           (const int32_t*)fresh.cells.as<int32_t>(), n, (int)C, d_cursor, fresh.order.as<int32_t>());
        MM_HIP(hipGetLastError());
    }
    MM_HIP(hipStreamSynchronize(st));
    mmiss_index::Partition& pt = ix->part;
    pt.C = fresh.C; pt.B = fresh.B; pt.in_cells = fresh.in_cells; pt.largest = fresh.largest; pt.empty = fresh.empty;
    pt.cn.swap(fresh.cn); pt.cells.swap(fresh.cells); pt.order.swap(fresh.order); pt.off.swap(fresh.off);
    pt.sizes.swap(fresh.sizes); pt.top_prefix.swap(fresh.top_prefix);
    pt.queries = 0; pt.scanned = 0;
    return MMISS_OK;
}

extern "C" int mmiss_index_partition_clear(mmiss_index* ix) {
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_partition_clear: null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_index_partition_clear");
    drop_partition(ix);
    return MMISS_OK;
}

extern "C" int mmiss_index_partition_info(mmiss_index* ix, int64_t out[8]) {
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_partition_info: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_index_partition_info");
    const mmiss_index::Partition& pt = ix->part;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (pt.C == 0) return MMISS_OK;
    out[0] = pt.C; out[1] = pt.B; out[2] = ix->count - pt.B; out[3] = pt.in_cells; out[4] = pt.largest; out[5] = pt.empty;
    out[6] = pt.queries; out[7] = pt.scanned;
    return MMISS_OK;
}

extern "C" int mmiss_index_partition_get(mmiss_index* ix, float* centres, int32_t* cells, int64_t cap_rows, int64_t* sizes) {
    const char* who = "mmiss_index_partition_get";
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "%s: null index", who);
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    MM_NEED_PARTITION(ix, who);
    const mmiss_index::Partition& pt = ix->part;
    if (cells && cap_rows < pt.B) MM_FAIL(MMISS_ERR_ARG, "%s: cap_rows = %lld for %lld cells", who, (long long)cap_rows, (long long)pt.B);
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    if (centres) MM_TRY(copy_any(centres, pt.cn.p, (size_t)pt.C * ix->dim * 4, st));
    if (cells) MM_TRY(copy_any(cells, pt.cells.p, (size_t)pt.B * 4, st));
    if (sizes) MM_TRY(copy_any(sizes, pt.sizes.data(), (size_t)pt.C * 8, st));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

namespace {

// A probed call under the handle's lock, its arguments checked (a partition included): the probed cells, the scan of their lists,
// the selection. Returns with the stream drained and host outputs delivered.
int probed_locked(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, int32_t nprobe, const uint64_t* require, const uint64_t* exclude,
                  int64_t* out_labels, float* out_dist, int32_t* out_count, int64_t* out_scanned, bool out_dev) {
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    mmiss_index::Partition& pt = ix->part;
    const int D = ix->dim;
    const int tail = (int)(ix->count - pt.B);
    const ProbePlan p = plan_probed(ix, Q, k, nprobe);
    // the scanned rows always go to a pinned block of their own (the partition's counter adds them up) and from there to the caller
    ResultBlock out;
    MM_TRY(out.stage(ix->pin, st, Q, k, out_dev, false, false, out_labels, out_dist, out_count, nullptr));
    MM_TRY(ix->swp_pin.ensure((size_t)Q * 8, st, (size_t)std::max(Q, 512) * 8));
    int64_t* const h_scn = ix->swp_pin.as<int64_t>();
    MM_TRY(upload_queries(ix, st, queries, Q));   // qn of every query of the call
    const uint64_t* d_req = require; const uint64_t* d_exc = exclude;   // host masks: [Q] required, then [Q] excluded in prb_mask
    MM_TRY(device_view(&d_req, (size_t)Q, ix->prb_mask, 0, (size_t)Q * 16, st));
    MM_TRY(device_view(&d_exc, (size_t)Q, ix->prb_mask, (size_t)Q * 8, (size_t)Q * 16, st));
    MM_TRY(ix->prb_cell.ensure((size_t)p.qchunk * std::max(p.NP, 1) * 4));
    MM_TRY(ix->prb_base.ensure((size_t)p.qchunk * (p.NP + 1) * 4));
    MM_TRY(ix->prb_total.ensure((size_t)p.qchunk * 4));
    MM_TRY(ix->prb_keys_a.ensure((size_t)p.qchunk * p.stride0 * 8));
    if (p.stride1) MM_TRY(ix->prb_keys_b.ensure((size_t)p.qchunk * p.stride1 * 8));
    const bool f16 = ix->dtype == MMISS_F16, f8 = ix->dtype == MMISS_F8;
    for (int q0 = 0; q0 < Q; q0 += p.qchunk) {
        const int Qc = std::min(p.qchunk, Q - q0);
        const float* qn = ix->qn.as<float>() + (size_t)q0 * D;
        {
            ProbeSelectArgs a{};
            a.qn = qn; a.cn = pt.cn.as<float>(); a.off = pt.off.as<int32_t>(); a.C = pt.C; a.D = D; a.NP = p.NP; a.tail = tail;
            a.probe_cell = ix->prb_cell.as<int32_t>(); a.probe_base = ix->prb_base.as<int32_t>(); a.total = ix->prb_total.as<int32_t>();
            MM_PROF("probe_select", st, 2.0 * Qc * pt.C * D, 4.0 * pt.C * D);
            hipLaunchKernelGGL(probe_select_kernel, dim3(Qc), dim3(1024), 0, st, a);
            MM_HIP(hipGetLastError());
        }
        {
            ListScanArgs a{};
            a.rows = ix->rows.p; a.inv = ix->inv.as<float>(); a.tags = ix->tags.as<uint64_t>(); a.qn = qn;
            a.req = d_req ? d_req + q0 : nullptr; a.exc = d_exc ? d_exc + q0 : nullptr;
            a.order = pt.order.as<int32_t>(); a.off = pt.off.as<int32_t>();
            a.probe_cell = ix->prb_cell.as<int32_t>(); a.probe_base = ix->prb_base.as<int32_t>(); a.total = ix->prb_total.as<int32_t>();
            a.D = D; a.NP = p.NP; a.share = p.share; a.B = pt.B; a.tail = tail;
            a.keys = ix->prb_keys_a.as<unsigned long long>(); a.stride = p.stride0;
            MM_PROF(f16 ? "list_scan_f16" : f8 ? "list_scan_f8" : "list_scan_f32", st, 2.0 * Qc * (double)p.bound * D,
                    (double)Qc * p.bound * (D * ix->elt + 12));
            with_storage(ix->dtype, [&](auto s) {
                hipLaunchKernelGGL(list_scan_kernel<typename decltype(s)::T>, dim3(p.splits, p.NP + 1, Qc), dim3(256), 0, st, a);
            });
            MM_HIP(hipGetLastError());
        }
        int64_t nb = p.bound;   // the most keys a query has at this level
        for (int l = 0; l < p.levels; ++l) {
            const bool last = l == p.levels - 1;
            const bool from_a = (l & 1) == 0;
            const int nseg = last ? 1 : (int)((nb + PROBE_SEG - 1) / PROBE_SEG);
            SegmentTopkArgs a{};
            a.in = from_a ? ix->prb_keys_a.as<unsigned long long>() : ix->prb_keys_b.as<unsigned long long>();
            a.out = from_a ? ix->prb_keys_b.as<unsigned long long>() : ix->prb_keys_a.as<unsigned long long>();
            a.in_stride = from_a ? p.stride0 : p.stride1; a.out_stride = from_a ? p.stride1 : p.stride0;
            a.total = ix->prb_total.as<int32_t>(); a.level = l; a.k = k;
            a.labels = ix->labels_d.as<int64_t>();
            a.out_labels = out.lab + (size_t)q0 * k; a.out_dist = out.dist + (size_t)q0 * k; a.out_count = out.cnt + q0; a.out_scanned = h_scn + q0;
            MM_PROF("segment_topk", st, 0.0, (double)Qc * nb * 8);
            if (last) hipLaunchKernelGGL(segment_topk_kernel<true>, dim3(1, Qc), dim3(1024), 0, st, a);
            else hipLaunchKernelGGL(segment_topk_kernel<false>, dim3(nseg, Qc), dim3(1024), 0, st, a);
            MM_HIP(hipGetLastError());
            nb = (int64_t)nseg * k;
        }
    }
    if (out_dev && out_scanned) MM_HIP(hipMemcpyAsync(out_scanned, h_scn, (size_t)Q * 8, hipMemcpyHostToDevice, st));
    MM_HIP(hipStreamSynchronize(st));
    out.deliver();
    if (!out_dev && out_scanned) memcpy(out_scanned, h_scn, (size_t)Q * 8);
    pt.queries += Q;
    for (int q = 0; q < Q; ++q) pt.scanned += h_scn[q];
    return MMISS_OK;
}

}  // namespace

extern "C" int mmiss_index_query_probed(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, int32_t nprobe, const uint64_t* require,
                                        const uint64_t* exclude, int64_t* out_labels, float* out_dist, int32_t* out_count, int64_t* out_scanned) {
    const char* who = "mmiss_index_query_probed";
    if (!ix || !queries || !out_labels || !out_dist || !out_count) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || nprobe < 1) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d nprobe=%d", who, Q, k, nprobe);
    if (k > PROBE_MAX_K) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: k = %d too large (max %d)", who, k, PROBE_MAX_K);
    bool out_dev = false;
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_scanned, &out_dev));
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    MM_NEED_PARTITION(ix, who);
    return probed_locked(ix, queries, Q, k, nprobe, require, exclude, out_labels, out_dist, out_count, out_scanned, out_dev);
}

// ================================================================================================ distinct results
// mmiss_index_query_distinct: the exact ranked list of each query — the flat / filtered query's (nprobe = 0) or the probed query's,
// k = pool, the very code of those calls writing into device scratch, so the list and the counters are theirs — and then the
// suppression stage (distinct_kernels.h): ONE launch for all queries, the greedy walk entirely on the device.
namespace {

int launch_distinct(mmiss_index* ix, hipStream_t st, const DistinctArgs& a, int Q) {
    const DistinctPlan p = plan_distinct(ix->dim, Q);
    const bool f16 = ix->dtype == MMISS_F16, f8 = ix->dtype == MMISS_F8;
    // (worst case: k rounds of pool dots per query)
    MM_PROF(f16 ? "distinct_f16" : f8 ? "distinct_f8" : "distinct_f32", st, 2.0 * Q * (double)a.k * a.pool * a.D, (double)Q * a.k * a.pool * a.D * ix->elt);
    typedef void (*Kernel)(DistinctArgs);
    const Kernel kern = with_storage(ix->dtype, [&](auto s) -> Kernel { return &distinct_kernel<typename decltype(s)::T>; });
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), p.lds));
    hipLaunchKernelGGL(kern, dim3(p.queries_per_launch), dim3(p.threads), p.lds, st, a);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

}  // namespace

extern "C" int mmiss_index_query_distinct(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, int32_t pool, float min_sep, int32_t nprobe,
                                          const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                                          int32_t* out_count, int32_t* out_dups, int32_t* out_listed) {
    const char* who = "mmiss_index_query_distinct";
    if (!ix || (Q > 0 && !queries) || !out_labels || !out_dist || !out_count) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 0 || k < 1 || pool < 1 || nprobe < 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d pool=%d nprobe=%d", who, Q, k, pool, nprobe);
    if (pool > PLAN_DISTINCT_MAX_POOL) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: pool = %d too large (max %d)", who, pool, PLAN_DISTINCT_MAX_POOL);
    if (k > pool) MM_FAIL(MMISS_ERR_ARG, "%s: k = %d above pool = %d", who, k, pool);
    if (min_sep != min_sep) MM_FAIL(MMISS_ERR_ARG, "%s: min_sep is NaN", who);
    bool out_dev = false, opt_dev = false;
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_dups, &out_dev));
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_listed, &opt_dev));
    if (Q == 0) return MMISS_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, who);
    if (nprobe >= 1) MM_NEED_PARTITION(ix, who);
    MM_TRY(mmiss_use_device(ix->device));
    hipStream_t st = ix->stream();
    // the list stage: [Q, pool] labels, [Q, pool] distances, [Q] counts in device scratch
    const size_t QP = (size_t)Q * pool, QK = (size_t)Q * k;
    MM_TRY(ix->dst_list.ensure(QP * 12 + (size_t)Q * 4));
    int64_t* const l_lab = ix->dst_list.as<int64_t>();
    float* const l_dist = reinterpret_cast<float*>(ix->dst_list.as<char>() + QP * 8);
    int32_t* const l_cnt = reinterpret_cast<int32_t*>(ix->dst_list.as<char>() + QP * 12);
    if (nprobe >= 1) {
        MM_TRY(probed_locked(ix, queries, Q, pool, nprobe, require, exclude, l_lab, l_dist, l_cnt, nullptr, true));
    } else {
        MM_TRY(query_begin_locked(ix, queries, Q, pool, require, exclude, l_lab, l_dist, l_cnt));
        MM_TRY(query_end_locked(ix));
    }
    // the suppression stage, into the caller's device buffers or into scratch on its way to the caller's host buffers
    DistinctArgs a{};
    a.rows = ix->rows.p; a.D = ix->dim; a.inv = ix->inv.as<float>(); a.labels = ix->labels_d.as<int64_t>(); a.N = ix->count;
    a.list_lab = l_lab; a.list_dist = l_dist; a.list_cnt = l_cnt; a.pool = pool; a.k = k; a.min_sep = min_sep;
    a.out_labels = out_labels; a.out_dist = out_dist; a.out_count = out_count; a.out_dups = out_dups; a.out_listed = out_listed;
    if (!out_dev) {
        MM_TRY(ix->dst_out.ensure(QK * 16 + (size_t)Q * 8));
        char* const b = ix->dst_out.as<char>();
        a.out_labels = reinterpret_cast<int64_t*>(b); a.out_dist = reinterpret_cast<float*>(b + QK * 8);
        a.out_dups = reinterpret_cast<int32_t*>(b + QK * 12); a.out_count = reinterpret_cast<int32_t*>(b + QK * 16);
        a.out_listed = a.out_count + Q;
    }
    MM_TRY(launch_distinct(ix, st, a, Q));
    if (!out_dev) {
        MM_HIP(hipMemcpyAsync(out_labels, a.out_labels, QK * 8, hipMemcpyDeviceToHost, st));
        MM_HIP(hipMemcpyAsync(out_dist, a.out_dist, QK * 4, hipMemcpyDeviceToHost, st));
        MM_HIP(hipMemcpyAsync(out_count, a.out_count, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
        if (out_dups) MM_HIP(hipMemcpyAsync(out_dups, a.out_dups, QK * 4, hipMemcpyDeviceToHost, st));
        if (out_listed) MM_HIP(hipMemcpyAsync(out_listed, a.out_listed, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    }
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// ================================================================================================ subset search
// mmiss_index_query_subset: the exact top-k among the rows whose labels the caller lists (subset_kernels.h). The list becomes a
// bitmap and then an ascending row list on the device, the scan scores every listed row against a block of queries at a time, and
// the probed call's selection picks the k best. No first pass, no guard, no partition: every listed row gets its canonical
// distance, and the guard's and the partition's counters stay as they are.
namespace {

SubsetPlan plan_subset(const mmiss_index* ix, int Q, int k, int64_t n_cand) {
    return plan_subset(ix->count, n_cand, ix->dim, Q, k, plan_options());
}

typedef void (*SubsetScanKernel)(SubsetScanArgs);
template <typename T> SubsetScanKernel subset_scan_kernel_for(int nqb) {
    switch (nqb) {
        case 16: return &subset_scan_kernel<T, 16>;
        case 8: return &subset_scan_kernel<T, 8>;
        case 4: return &subset_scan_kernel<T, 4>;
        case 2: return &subset_scan_kernel<T, 2>;
        default: return &subset_scan_kernel<T, 1>;
    }
}

// stages 1 and 2: the caller's list -> sub_rows (ascending rows of S) and prb_total[0 .. nq) = |S|
int subset_rows(mmiss_index* ix, hipStream_t st, const SubsetPlan& p, const int64_t* d_cand, int64_t n_cand, int nq) {
    uint32_t* const bitmap = ix->sub_bitmap.as<uint32_t>();
    int32_t* const blk = ix->sub_blk.as<int32_t>();
    MM_HIP(hipMemsetAsync(bitmap, 0, (size_t)p.words * 4, st));
    {
        MM_PROF("subset_mark", st, 0.0, 8.0 * n_cand);
        hipLaunchKernelGGL(subset_mark_kernel, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, st, d_cand, n_cand,
                           (const int64_t*)ix->labels_d.as<int64_t>(), ix->count, bitmap);
        MM_HIP(hipGetLastError());
    }
    MM_PROF("subset_compact", st, 0.0, 8.0 * p.words + 4.0 * p.bound);
    hipLaunchKernelGGL(subset_count_kernel, dim3(p.blocks), dim3(SUBSET_BLOCK_THREADS), 0, st, (const uint32_t*)bitmap, p.words, blk);
    MM_HIP(hipGetLastError());
    hipLaunchKernelGGL(subset_offsets_kernel, dim3(1), dim3(SUBSET_BLOCK_THREADS), 0, st, blk, p.blocks, ix->prb_total.as<int32_t>(), nq);
    MM_HIP(hipGetLastError());
    hipLaunchKernelGGL(subset_scatter_kernel, dim3(p.blocks), dim3(SUBSET_BLOCK_THREADS), 0, st, (const uint32_t*)bitmap, p.words,
                       (const int32_t*)blk, ix->sub_rows.as<int32_t>(), p.bound);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

}  // namespace

extern "C" int mmiss_index_query_subset(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, const int64_t* cand_labels, int64_t n_cand,
                                        const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                                        int32_t* out_count, int64_t* out_matched) {
    const char* who = "mmiss_index_query_subset";
    if (!ix || !queries || !out_labels || !out_dist || !out_count) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || n_cand < 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d n_cand=%lld", who, Q, k, (long long)n_cand);
    if (n_cand > 0 && !cand_labels) MM_FAIL(MMISS_ERR_ARG, "%s: null cand_labels for %lld labels", who, (long long)n_cand);
    if (k > PROBE_MAX_K) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: k = %d too large (max %d)", who, k, PROBE_MAX_K);
    if (n_cand > INT32_MAX) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: n_cand = %lld too large (max %d)", who, (long long)n_cand, INT32_MAX);
    bool out_dev = false;
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_matched, &out_dev));
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    const int D = ix->dim;
    const SubsetPlan p = plan_subset(ix, Q, k, n_cand);
    ResultBlock out;
    MM_TRY(out.stage(ix->pin, st, Q, k, out_dev, true, false, out_labels, out_dist, out_count, out_matched));
    MM_TRY(upload_queries(ix, st, queries, Q));   // qn of every query of the call
    const uint64_t* d_req = require; const uint64_t* d_exc = exclude;   // host masks: [Q] required, then [Q] excluded in prb_mask
    MM_TRY(device_view(&d_req, (size_t)Q, ix->prb_mask, 0, (size_t)Q * 16, st));
    MM_TRY(device_view(&d_exc, (size_t)Q, ix->prb_mask, (size_t)Q * 8, (size_t)Q * 16, st));
    MM_TRY(ix->prb_total.ensure((size_t)p.qchunk * 4));
    MM_TRY(ix->prb_keys_a.ensure((size_t)p.qchunk * p.stride0 * 8));
    if (p.stride1) MM_TRY(ix->prb_keys_b.ensure((size_t)p.qchunk * p.stride1 * 8));
    if (p.bound > 0) {
        const int64_t* d_cand = cand_labels;
        MM_TRY(device_view(&d_cand, (size_t)n_cand, ix->sub_cand, 0, (size_t)n_cand * 8, st));
        MM_TRY(ix->sub_bitmap.ensure((size_t)p.words * 4));
        MM_TRY(ix->sub_blk.ensure((size_t)p.blocks * 4));
        MM_TRY(ix->sub_rows.ensure((size_t)p.bound * 4));
        MM_TRY(subset_rows(ix, st, p, d_cand, n_cand, p.qchunk));
    } else {
        MM_HIP(hipMemsetAsync(ix->prb_total.p, 0, (size_t)p.qchunk * 4, st));   // an empty list or an empty index: |S| = 0
    }
    const bool f16 = ix->dtype == MMISS_F16, f8 = ix->dtype == MMISS_F8;
    for (int q0 = 0; q0 < Q; q0 += p.qchunk) {
        const int Qc = std::min(p.qchunk, Q - q0);
        if (p.bound > 0) {
            SubsetScanArgs a{};
            a.rows = ix->rows.p; a.inv = ix->inv.as<float>(); a.tags = ix->tags.as<uint64_t>();
            a.qn = ix->qn.as<float>() + (size_t)q0 * D;
            a.req = d_req ? d_req + q0 : nullptr; a.exc = d_exc ? d_exc + q0 : nullptr;
            a.list = ix->sub_rows.as<int32_t>(); a.total = ix->prb_total.as<int32_t>();
            a.Q = Qc; a.D = D; a.share = p.share;
            a.keys = ix->prb_keys_a.as<unsigned long long>(); a.stride = p.stride0;
            const int nqb = subset_block_for(p.qblock, Qc);
            const int qblocks = (Qc + nqb - 1) / nqb;
            // (the rows are read once per query block)
            MM_PROF(f16 ? "subset_scan_f16" : f8 ? "subset_scan_f8" : "subset_scan_f32", st, 2.0 * Qc * (double)p.bound * D,
                    (double)qblocks * p.bound * (D * ix->elt + 12) + 8.0 * Qc * p.bound);
            const SubsetScanKernel kern = with_storage(ix->dtype, [&](auto s) { return subset_scan_kernel_for<typename decltype(s)::T>(nqb); });
            const int lds = subset_scan_lds_bytes(D, nqb);
            MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds));
            hipLaunchKernelGGL(kern, dim3(p.splits, qblocks), dim3(256), lds, st, a);
            MM_HIP(hipGetLastError());
        }
        int64_t nb = p.bound;   // the most keys a query has at this level
        for (int l = 0; l < p.levels; ++l) {
            const bool last = l == p.levels - 1;
            const bool from_a = (l & 1) == 0;
            const int nseg = last ? 1 : (int)((nb + PROBE_SEG - 1) / PROBE_SEG);
            SegmentTopkArgs a{};
            a.in = from_a ? ix->prb_keys_a.as<unsigned long long>() : ix->prb_keys_b.as<unsigned long long>();
            a.out = from_a ? ix->prb_keys_b.as<unsigned long long>() : ix->prb_keys_a.as<unsigned long long>();
            a.in_stride = from_a ? p.stride0 : p.stride1; a.out_stride = from_a ? p.stride1 : p.stride0;
            a.total = ix->prb_total.as<int32_t>(); a.level = l; a.k = k;
            a.labels = ix->labels_d.as<int64_t>();
            a.out_labels = out.lab + (size_t)q0 * k; a.out_dist = out.dist + (size_t)q0 * k; a.out_count = out.cnt + q0;
            a.out_scanned = out.tot ? out.tot + q0 : nullptr;
            MM_PROF("segment_topk", st, 0.0, (double)Qc * nb * 8);
            if (last) hipLaunchKernelGGL(segment_topk_kernel<true>, dim3(1, Qc), dim3(1024), 0, st, a);
            else hipLaunchKernelGGL(segment_topk_kernel<false>, dim3(nseg, Qc), dim3(1024), 0, st, a);
            MM_HIP(hipGetLastError());
            nb = (int64_t)nseg * k;
        }
    }
    MM_HIP(hipStreamSynchronize(st));
    out.deliver();
    return MMISS_OK;
}

// mmiss_debug.h: how a subset call of this shape would run on the index as it stands (plan_subset, nothing launched).
extern "C" int mmiss_dbg_index_subset_plan(mmiss_index* ix, int32_t Q, int32_t k, int64_t n_cand, int32_t* out) {
    const char* who = "mmiss_dbg_index_subset_plan";
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || k > PROBE_MAX_K || n_cand < 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d n_cand=%lld", who, Q, k, (long long)n_cand);
    std::lock_guard<std::mutex> lk(ix->mu);
    const SubsetPlan p = plan_subset(ix, Q, k, n_cand);
    auto i32 = [](int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); };
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[0] = i32(p.bound); out[1] = PROBE_SEG; out[2] = p.levels; out[3] = i32(p.stride0); out[4] = i32(p.stride1);
    out[5] = p.qchunk; out[6] = p.chunks; out[7] = p.qblock; out[8] = p.lds; out[9] = p.share; out[10] = p.splits;
    out[11] = SUBSET_ROWS_PER_TRIP; out[12] = p.blocks; out[13] = SUBSET_BLOCK_ROWS;
    out[14] = subset_block_for(p.qblock, std::min(Q, p.qchunk)); out[15] = subset_block_for(p.qblock, Q - (p.chunks - 1) * p.qchunk);
    return MMISS_OK;
}

// ================================================================================================ grouped search
// mmiss_index_query_grouped: the exact k nearest groups of each query, each by its best row (grouped_kernels.h). Stage 1 is the
// flat / filtered query at k = pool, the very code of those calls writing into device scratch (as the distinct call runs it), so the
// list and the guard counters are theirs. Stage 2 walks every list in ONE launch and flags the queries whose list did not settle
// the answer; the host looks at the flags once. Stage 3, for those queries only and compacted: a scan of every row into a table of
// one slot per group (an atomic minimum of the (distance, row) keys), the probed call's selection over the table, and the resolve
// kernel that puts the heads into the queries' own output rows. Stages 2 and 3 count nothing.
namespace {

GroupedPlan plan_grouped(const mmiss_index* ix, int Qx, int k, int pool) {
    return plan_grouped(ix->count, ix->group_hwm, ix->dim, Qx, k, pool, plan_options());
}

typedef void (*GroupedScanKernel)(GroupedScanArgs);
template <typename T> GroupedScanKernel grouped_scan_kernel_for(int nqb) {
    switch (nqb) {
        case 16: return &grouped_scan_kernel<T, 16>;
        case 8: return &grouped_scan_kernel<T, 8>;
        case 4: return &grouped_scan_kernel<T, 4>;
        case 2: return &grouped_scan_kernel<T, 2>;
        default: return &grouped_scan_kernel<T, 1>;
    }
}

// *col: the group column on the device, uploaded from the host mirror if that changed since the last upload; null while no row has
// had a group since the last clear or load (the kernels read null as "every row ungrouped")
int group_column(mmiss_index* ix, hipStream_t st, const int32_t** col) {
    *col = nullptr;
    if (ix->group_hwm == 0 || ix->count == 0) return MMISS_OK;
    if (ix->groups_dirty) {
        MM_TRY(ix->grp_col.ensure((size_t)ix->count * 4));   // (every grouped call returns finished: nothing queued reads the old one)
        MM_HIP(hipMemcpyAsync(ix->grp_col.p, ix->groups_h.data(), (size_t)ix->count * 4, hipMemcpyHostToDevice, st));
        MM_HIP(hipStreamSynchronize(st));
        ix->groups_dirty = false;
    }
    *col = ix->grp_col.as<int32_t>();
    return MMISS_OK;
}

// Stage 3 for the flagged queries `which` (indices into the call): returns with everything queued on st
int grouped_exhaustive(mmiss_index* ix, hipStream_t st, const std::vector<int32_t>& which, int Q, int k, int pool, const int32_t* col,
                       const uint64_t* require, const uint64_t* exclude, int64_t* o_lab, float* o_dist, int32_t* o_grp, int32_t* o_cnt,
                       int32_t* o_route) {
    const int Qf = (int)which.size(), D = ix->dim;
    const GroupedPlan p = plan_grouped(ix, Qf, k, pool);
    MM_TRY(ix->grp_map.ensure((size_t)Qf * 4));
    MM_HIP(hipMemcpyAsync(ix->grp_map.p, which.data(), (size_t)Qf * 4, hipMemcpyHostToDevice, st));   // (`which` outlives the call's last wait)
    const uint64_t* d_req = require; const uint64_t* d_exc = exclude;   // host masks: [Q] required, then [Q] excluded in prb_mask
    MM_TRY(device_view(&d_req, (size_t)Q, ix->prb_mask, 0, (size_t)Q * 16, st));
    MM_TRY(device_view(&d_exc, (size_t)Q, ix->prb_mask, (size_t)Q * 8, (size_t)Q * 16, st));
    MM_TRY(ix->prb_total.ensure((size_t)p.qchunk * 4));
    MM_TRY(ix->prb_keys_a.ensure((size_t)p.qchunk * p.stride0 * 8));
    if (p.stride1) MM_TRY(ix->prb_keys_b.ensure((size_t)p.qchunk * p.stride1 * 8));
    const size_t CK = (size_t)p.qchunk * k;
    MM_TRY(ix->grp_sel.ensure(CK * 12 + (size_t)p.qchunk * 4));
    int64_t* const s_lab = ix->grp_sel.as<int64_t>();
    float* const s_dist = reinterpret_cast<float*>(ix->grp_sel.as<char>() + CK * 8);
    int32_t* const s_cnt = reinterpret_cast<int32_t*>(ix->grp_sel.as<char>() + CK * 12);
    MM_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ix->prb_total.p), (int)p.table, (size_t)p.qchunk, st));   // every query: G + count slots
    const bool f16 = ix->dtype == MMISS_F16, f8 = ix->dtype == MMISS_F8;
    for (int c0 = 0; c0 < Qf; c0 += p.qchunk) {
        const int Qc = std::min(p.qchunk, Qf - c0);
        const int32_t* qmap = ix->grp_map.as<int32_t>() + c0;
        MM_HIP(hipMemsetAsync(ix->prb_keys_a.p, 0xff, (size_t)Qc * p.stride0 * 8, st));   // PROBE_KEY_NONE in every slot
        {
            GroupedScanArgs a{};
            a.rows = ix->rows.p; a.inv = ix->inv.as<float>(); a.tags = ix->tags.as<uint64_t>(); a.groups = col;
            a.qn = ix->qn.as<float>(); a.req = d_req; a.exc = d_exc; a.qmap = qmap;
            a.Qc = Qc; a.D = D; a.N = (int)ix->count; a.G = (int)ix->group_hwm; a.share = p.share;
            a.table = ix->prb_keys_a.as<unsigned long long>(); a.stride = p.stride0;
            const int nqb = subset_block_for(p.qblock, Qc);
            const int qblocks = (Qc + nqb - 1) / nqb;
            MM_PROF(f16 ? "grouped_scan_f16" : f8 ? "grouped_scan_f8" : "grouped_scan_f32", st, 2.0 * Qc * (double)ix->count * D,
                    (double)qblocks * ix->count * (D * ix->elt + 12) + 8.0 * Qc * ix->count);
            const GroupedScanKernel kern = with_storage(ix->dtype, [&](auto s) { return grouped_scan_kernel_for<typename decltype(s)::T>(nqb); });
            const int lds = grouped_scan_lds_bytes(D, nqb);
            MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds));
            hipLaunchKernelGGL(kern, dim3(p.splits, qblocks), dim3(256), lds, st, a);
            MM_HIP(hipGetLastError());
        }
        int64_t nb = p.table;   // the keys a query has at this level
        for (int l = 0; l < p.levels; ++l) {
            const bool last = l == p.levels - 1;
            const bool from_a = (l & 1) == 0;
            const int nseg = last ? 1 : (int)((nb + PROBE_SEG - 1) / PROBE_SEG);
            SegmentTopkArgs a{};
            a.in = from_a ? ix->prb_keys_a.as<unsigned long long>() : ix->prb_keys_b.as<unsigned long long>();
            a.out = from_a ? ix->prb_keys_b.as<unsigned long long>() : ix->prb_keys_a.as<unsigned long long>();
            a.in_stride = from_a ? p.stride0 : p.stride1; a.out_stride = from_a ? p.stride1 : p.stride0;
            a.total = ix->prb_total.as<int32_t>(); a.level = l; a.k = k;
            a.labels = ix->labels_d.as<int64_t>();
            a.out_labels = s_lab; a.out_dist = s_dist; a.out_count = s_cnt; a.out_scanned = nullptr;
            MM_PROF("segment_topk", st, 0.0, (double)Qc * nb * 8);
            if (last) hipLaunchKernelGGL(segment_topk_kernel<true>, dim3(1, Qc), dim3(1024), 0, st, a);
            else hipLaunchKernelGGL(segment_topk_kernel<false>, dim3(nseg, Qc), dim3(1024), 0, st, a);
            MM_HIP(hipGetLastError());
            nb = (int64_t)nseg * k;
        }
        {
            GroupedResolveArgs a{};
            a.labels = ix->labels_d.as<int64_t>(); a.N = ix->count; a.groups = col; a.qmap = qmap;
            a.sel_labels = s_lab; a.sel_dist = s_dist; a.sel_count = s_cnt; a.k = k;
            a.out_labels = o_lab; a.out_dist = o_dist; a.out_group = o_grp; a.out_count = o_cnt; a.out_route = o_route;
            MM_PROF("grouped_resolve", st, 0.0, (double)Qc * k * 32);
            hipLaunchKernelGGL(grouped_resolve_kernel, dim3(Qc), dim3(256), 0, st, a);
            MM_HIP(hipGetLastError());
        }
    }
    return MMISS_OK;
}

}  // namespace

extern "C" int mmiss_index_query_grouped(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, int32_t pool, const uint64_t* require,
                                         const uint64_t* exclude, int64_t* out_labels, float* out_dist, int32_t* out_group,
                                         int32_t* out_count, int32_t* out_route) {
    const char* who = "mmiss_index_query_grouped";
    if (!ix || !queries || !out_labels || !out_dist || !out_group || !out_count) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || pool < 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d pool=%d", who, Q, k, pool);
    if (k > PROBE_MAX_K) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: k = %d too large (max %d)", who, k, PROBE_MAX_K);
    if (pool > PLAN_GROUPED_MAX_POOL) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: pool = %d too large (max %d)", who, pool, PLAN_GROUPED_MAX_POOL);
    if (pool != 0 && pool < k) MM_FAIL(MMISS_ERR_ARG, "%s: pool = %d below k = %d", who, pool, k);
    bool out_dev = false, opt_dev = false;
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_group, &out_dev));
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_route, &opt_dev));
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    if (ix->group_hwm + ix->count > (int64_t)INT32_MAX)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: %lld groups and %lld rows exceed 2^31 - 1 table slots", who, (long long)ix->group_hwm, (long long)ix->count);
    const int P = pool > 0 ? pool : grouped_default_pool(k);
    const int32_t* col = nullptr;
    MM_TRY(group_column(ix, st, &col));
    // stage 1, the list: [Q, P] labels, [Q, P] distances, [Q] counts in device scratch
    const size_t QP = (size_t)Q * P, QK = (size_t)Q * k;
    MM_TRY(ix->grp_list.ensure(QP * 12 + (size_t)Q * 4));
    int64_t* const l_lab = ix->grp_list.as<int64_t>();
    float* const l_dist = reinterpret_cast<float*>(ix->grp_list.as<char>() + QP * 8);
    int32_t* const l_cnt = reinterpret_cast<int32_t*>(ix->grp_list.as<char>() + QP * 12);
    MM_TRY(query_begin_locked(ix, queries, Q, P, require, exclude, l_lab, l_dist, l_cnt));
    MM_TRY(query_end_locked(ix));
    // stage 2, the walk: into the caller's device buffers, or into scratch on its way to the caller's host buffers
    int64_t* o_lab = out_labels; float* o_dist = out_dist; int32_t* o_grp = out_group; int32_t* o_cnt = out_count; int32_t* o_route = out_route;
    if (!out_dev) {
        MM_TRY(ix->grp_out.ensure(QK * 16 + (size_t)Q * 8));
        char* const b = ix->grp_out.as<char>();
        o_lab = reinterpret_cast<int64_t*>(b); o_dist = reinterpret_cast<float*>(b + QK * 8); o_grp = reinterpret_cast<int32_t*>(b + QK * 12);
        o_cnt = reinterpret_cast<int32_t*>(b + QK * 16); o_route = o_cnt + Q;
    }
    MM_TRY(ix->grp_pin.ensure((size_t)Q * 4, st, (size_t)std::max(Q, 1024) * 4));
    int32_t* const complete = ix->grp_pin.as<int32_t>();
    {
        GroupedWalkArgs a{};
        a.labels = ix->labels_d.as<int64_t>(); a.N = ix->count; a.groups = col;
        a.list_lab = l_lab; a.list_dist = l_dist; a.list_cnt = l_cnt; a.pool = P; a.k = k;
        a.out_labels = o_lab; a.out_dist = o_dist; a.out_group = o_grp; a.out_count = o_cnt; a.out_route = o_route; a.complete = complete;
        MM_PROF("grouped_walk", st, 0.0, (double)Q * P * 12);
        hipLaunchKernelGGL(grouped_walk_kernel, dim3(Q), dim3(GROUPED_THREADS), 0, st, a);
        MM_HIP(hipGetLastError());
    }
    MM_HIP(hipStreamSynchronize(st));   // the one host look: which walks did not settle their query
    std::vector<int32_t> which;
    for (int q = 0; q < Q; ++q)
        if (!complete[q]) which.push_back(q);
    // stage 3, the exhaustive route
    if (!which.empty()) MM_TRY(grouped_exhaustive(ix, st, which, Q, k, pool, col, require, exclude, o_lab, o_dist, o_grp, o_cnt, o_route));
    if (!out_dev) {
        MM_HIP(hipMemcpyAsync(out_labels, o_lab, QK * 8, hipMemcpyDeviceToHost, st));
        MM_HIP(hipMemcpyAsync(out_dist, o_dist, QK * 4, hipMemcpyDeviceToHost, st));
        MM_HIP(hipMemcpyAsync(out_group, o_grp, QK * 4, hipMemcpyDeviceToHost, st));
        MM_HIP(hipMemcpyAsync(out_count, o_cnt, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
        if (out_route) MM_HIP(hipMemcpyAsync(out_route, o_route, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    }
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// mmiss_debug.h: how a grouped call of this shape would run on the index as it stands (plan_grouped, nothing launched).
extern "C" int mmiss_dbg_index_grouped_plan(mmiss_index* ix, int32_t Q, int32_t k, int32_t pool, int32_t* out) {
    const char* who = "mmiss_dbg_index_grouped_plan";
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || k > PROBE_MAX_K || pool < 0 || pool > PLAN_GROUPED_MAX_POOL || (pool != 0 && pool < k))
        MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d pool=%d", who, Q, k, pool);
    std::lock_guard<std::mutex> lk(ix->mu);
    const GroupedPlan p = plan_grouped(ix, Q, k, pool);
    auto i32 = [](int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); };
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[0] = p.pool; out[1] = p.walk_threads; out[2] = p.walk_lds; out[3] = i32(p.table); out[4] = PROBE_SEG; out[5] = p.levels;
    out[6] = i32(p.stride0); out[7] = i32(p.stride1); out[8] = p.qchunk; out[9] = p.chunks; out[10] = p.qblock; out[11] = p.lds;
    out[12] = p.share; out[13] = p.splits;
    out[14] = subset_block_for(p.qblock, std::min(Q, p.qchunk)); out[15] = subset_block_for(p.qblock, Q - (p.chunks - 1) * p.qchunk);
    return MMISS_OK;
}

// ================================================================================================ search after
// mmiss_index_query_after: the exact next k of every query's ranking behind its cursor (after_kernels.h). The subset call's
// stages with two differences: without a list nothing is marked or compacted (the dense scan's position is the row), and the
// scan's admission adds the radius and the cursor and counts what it admits (out_remaining).
namespace {

AfterPlan plan_after(const mmiss_index* ix, int Q, int k, int64_t n_cand) {
    return plan_after(ix->count, n_cand, ix->dim, Q, k, plan_options());
}

typedef void (*AfterScanKernel)(AfterScanArgs);
template <typename T, bool DENSE> AfterScanKernel after_scan_kernel_for(int nqb) {
    switch (nqb) {
        case 16: return &after_scan_kernel<T, 16, DENSE>;
        case 8: return &after_scan_kernel<T, 8, DENSE>;
        case 4: return &after_scan_kernel<T, 4, DENSE>;
        case 2: return &after_scan_kernel<T, 2, DENSE>;
        default: return &after_scan_kernel<T, 1, DENSE>;
    }
}

// aft_cur of a call of Q queries, in bytes from its start: the remaining counts and the caller's labels (8 bytes each), the
// resolved cursors (16), the caller's distances and radii (4 each)
struct AfterLayout {
    size_t remaining, label, cur, dist, radius, need;
};
AfterLayout after_layout(int Q) {
    AfterLayout l;
    l.remaining = 0; l.label = (size_t)Q * 8; l.cur = (size_t)Q * 16; l.dist = (size_t)Q * 32; l.radius = (size_t)Q * 36;
    l.need = (size_t)Q * 40;
    return l;
}

}  // namespace

extern "C" int mmiss_index_query_after(mmiss_index* ix, const float* queries, int32_t Q, int32_t k, const float* after_dist,
                                       const int64_t* after_label, const float* max_dist, const int64_t* cand_labels, int64_t n_cand,
                                       const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                                       int32_t* out_count, int64_t* out_remaining) {
    const char* who = "mmiss_index_query_after";
    if (!ix || !queries || !after_dist || !after_label || !out_labels || !out_dist || !out_count) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || n_cand < 0) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d n_cand=%lld", who, Q, k, (long long)n_cand);
    if (n_cand > 0 && !cand_labels) MM_FAIL(MMISS_ERR_ARG, "%s: null cand_labels for %lld labels", who, (long long)n_cand);
    if (k > PROBE_MAX_K) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: k = %d too large (max %d)", who, k, PROBE_MAX_K);
    if (n_cand > INT32_MAX) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: n_cand = %lld too large (max %d)", who, (long long)n_cand, INT32_MAX);
    bool out_dev = false;
    MM_TRY(outputs_all_host_or_all_device(who, out_labels, out_dist, out_count, out_remaining, &out_dev));
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, who, &st));
    if (ix->count > INT32_MAX) MM_FAIL(MMISS_ERR_UNSUPPORTED, "%s: %lld rows (max %d)", who, (long long)ix->count, INT32_MAX);
    const int D = ix->dim;
    const bool listed = cand_labels != nullptr;
    const AfterPlan p = plan_after(ix, Q, k, listed ? n_cand : -1);
    ResultBlock out;
    MM_TRY(out.stage(ix->pin, st, Q, k, out_dev, true, false, out_labels, out_dist, out_count, out_remaining));
    MM_TRY(upload_queries(ix, st, queries, Q));   // qn of every query of the call
    const uint64_t* d_req = require; const uint64_t* d_exc = exclude;   // host masks: [Q] required, then [Q] excluded in prb_mask
    MM_TRY(device_view(&d_req, (size_t)Q, ix->prb_mask, 0, (size_t)Q * 16, st));
    MM_TRY(device_view(&d_exc, (size_t)Q, ix->prb_mask, (size_t)Q * 8, (size_t)Q * 16, st));
    const AfterLayout al = after_layout(Q);
    MM_TRY(ix->aft_cur.ensure(al.need));
    const float* d_ad = after_dist; const int64_t* d_al = after_label; const float* d_md = max_dist;
    MM_TRY(device_view(&d_ad, (size_t)Q, ix->aft_cur, al.dist, al.need, st));
    MM_TRY(device_view(&d_al, (size_t)Q, ix->aft_cur, al.label, al.need, st));
    MM_TRY(device_view(&d_md, (size_t)Q, ix->aft_cur, al.radius, al.need, st));
    AfterCursor* const d_cur = reinterpret_cast<AfterCursor*>(ix->aft_cur.as<char>() + al.cur);
    unsigned long long* const d_rem = reinterpret_cast<unsigned long long*>(ix->aft_cur.as<char>() + al.remaining);
    MM_TRY(ix->prb_total.ensure((size_t)p.qchunk * 4));
    MM_TRY(ix->prb_keys_a.ensure((size_t)p.qchunk * p.stride0 * 8));
    if (p.stride1) MM_TRY(ix->prb_keys_b.ensure((size_t)p.qchunk * p.stride1 * 8));
    {
        // (a dense call's totals are the row count, written here; a listed call's come from the compaction below)
        MM_PROF("after_resolve", st, 0.0, 40.0 * Q);
        hipLaunchKernelGGL(after_resolve_kernel, dim3((Q + 255) / 256), dim3(256), 0, st, d_ad, d_al, d_md,
                           (const int64_t*)ix->labels_d.as<int64_t>(), ix->count, Q, d_cur, d_rem,
                           p.dense ? ix->prb_total.as<int32_t>() : (int32_t*)nullptr, p.qchunk);
        MM_HIP(hipGetLastError());
    }
    if (!p.dense) {
        if (p.bound > 0) {
            const int64_t* d_cand = cand_labels;
            MM_TRY(device_view(&d_cand, (size_t)n_cand, ix->sub_cand, 0, (size_t)n_cand * 8, st));
            MM_TRY(ix->sub_bitmap.ensure((size_t)p.words * 4));
            MM_TRY(ix->sub_blk.ensure((size_t)p.blocks * 4));
            MM_TRY(ix->sub_rows.ensure((size_t)p.bound * 4));
            MM_TRY(subset_rows(ix, st, p, d_cand, n_cand, p.qchunk));
        } else {
            MM_HIP(hipMemsetAsync(ix->prb_total.p, 0, (size_t)p.qchunk * 4, st));   // an empty list or an empty index: |S| = 0
        }
    }
    const bool f16 = ix->dtype == MMISS_F16, f8 = ix->dtype == MMISS_F8;
    for (int q0 = 0; q0 < Q; q0 += p.qchunk) {
        const int Qc = std::min(p.qchunk, Q - q0);
        if (p.bound > 0) {
            AfterScanArgs aa{};
            SubsetScanArgs& a = aa.s;
            a.rows = ix->rows.p; a.inv = ix->inv.as<float>(); a.tags = ix->tags.as<uint64_t>();
            a.qn = ix->qn.as<float>() + (size_t)q0 * D;
            a.req = d_req ? d_req + q0 : nullptr; a.exc = d_exc ? d_exc + q0 : nullptr;
            a.list = p.dense ? nullptr : ix->sub_rows.as<int32_t>(); a.total = ix->prb_total.as<int32_t>();
            a.Q = Qc; a.D = D; a.share = p.share;
            a.keys = ix->prb_keys_a.as<unsigned long long>(); a.stride = p.stride0;
            aa.cur = d_cur + q0; aa.remaining = d_rem + q0;
            const int nqb = subset_block_for(p.qblock, Qc);
            const int qblocks = (Qc + nqb - 1) / nqb;
            MM_PROF(f16 ? "after_scan_f16" : f8 ? "after_scan_f8" : "after_scan_f32", st, 2.0 * Qc * (double)p.bound * D,
                    (double)qblocks * p.bound * (D * ix->elt + 12) + 8.0 * Qc * p.bound);
            const AfterScanKernel kern = with_storage(ix->dtype, [&](auto s) {
                using T = typename decltype(s)::T;
                return p.dense ? after_scan_kernel_for<T, true>(nqb) : after_scan_kernel_for<T, false>(nqb);
            });
            const int lds = subset_scan_lds_bytes(D, nqb);
            MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds));
            hipLaunchKernelGGL(kern, dim3(p.splits, qblocks), dim3(256), lds, st, aa);
            MM_HIP(hipGetLastError());
        }
        int64_t nb = p.bound;   // the most keys a query has at this level
        for (int l = 0; l < p.levels; ++l) {
            const bool last = l == p.levels - 1;
            const bool from_a = (l & 1) == 0;
            const int nseg = last ? 1 : (int)((nb + PROBE_SEG - 1) / PROBE_SEG);
            SegmentTopkArgs a{};
            a.in = from_a ? ix->prb_keys_a.as<unsigned long long>() : ix->prb_keys_b.as<unsigned long long>();
            a.out = from_a ? ix->prb_keys_b.as<unsigned long long>() : ix->prb_keys_a.as<unsigned long long>();
            a.in_stride = from_a ? p.stride0 : p.stride1; a.out_stride = from_a ? p.stride1 : p.stride0;
            a.total = ix->prb_total.as<int32_t>(); a.level = l; a.k = k;
            a.labels = ix->labels_d.as<int64_t>();
            a.out_labels = out.lab + (size_t)q0 * k; a.out_dist = out.dist + (size_t)q0 * k; a.out_count = out.cnt + q0;
            a.out_scanned = nullptr;
            MM_PROF("segment_topk", st, 0.0, (double)Qc * nb * 8);
            if (last) hipLaunchKernelGGL(segment_topk_kernel<true>, dim3(1, Qc), dim3(1024), 0, st, a);
            else hipLaunchKernelGGL(segment_topk_kernel<false>, dim3(nseg, Qc), dim3(1024), 0, st, a);
            MM_HIP(hipGetLastError());
            nb = (int64_t)nseg * k;
        }
    }
    // the remaining counts leave by a copy of their own: into the caller's device array, or into the result block's pinned totals
    if (out.tot) MM_HIP(hipMemcpyAsync(out.tot, d_rem, (size_t)Q * 8, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    MM_HIP(hipStreamSynchronize(st));
    out.deliver();
    return MMISS_OK;
}

// mmiss_debug.h: how a continuation call of this shape would run on the index as it stands (plan_after, nothing launched).
extern "C" int mmiss_dbg_index_after_plan(mmiss_index* ix, int32_t Q, int32_t k, int64_t n_cand, int32_t* out) {
    const char* who = "mmiss_dbg_index_after_plan";
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || k > PROBE_MAX_K) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d", who, Q, k);
    std::lock_guard<std::mutex> lk(ix->mu);
    const AfterPlan p = plan_after(ix, Q, k, n_cand < 0 ? -1 : n_cand);
    auto i32 = [](int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); };
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[0] = i32(p.bound); out[1] = PROBE_SEG; out[2] = p.levels; out[3] = i32(p.stride0); out[4] = i32(p.stride1);
    out[5] = p.qchunk; out[6] = p.chunks; out[7] = p.qblock; out[8] = p.lds; out[9] = p.share; out[10] = p.splits;
    out[11] = SUBSET_ROWS_PER_TRIP; out[12] = p.blocks; out[13] = p.dense ? 1 : 0;
    out[14] = subset_block_for(p.qblock, std::min(Q, p.qchunk)); out[15] = subset_block_for(p.qblock, Q - (p.chunks - 1) * p.qchunk);
    return MMISS_OK;
}

// mmiss_debug.h: the layout of the suppression stage of a distinct call of Q queries on this index (plan_distinct, nothing launched).
extern "C" int mmiss_dbg_index_distinct_plan(mmiss_index* ix, int32_t Q, int32_t* out) {
    const char* who = "mmiss_dbg_index_distinct_plan";
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d", who, Q);
    const DistinctPlan p = plan_distinct(ix->dim, Q);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = p.rows_per_trip; out[1] = p.threads; out[2] = p.lds; out[3] = p.queries_per_launch; out[4] = p.launches;
    out[5] = PLAN_DISTINCT_MAX_POOL;
    return MMISS_OK;
}

// mmiss_debug.h: how a probed call of this shape would run on the partition as it stands (plan_probed, nothing launched).
extern "C" int mmiss_dbg_index_probe_plan(mmiss_index* ix, int32_t Q, int32_t k, int32_t nprobe, int32_t* out) {
    const char* who = "mmiss_dbg_index_probe_plan";
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (Q < 1 || k < 1 || k > PROBE_MAX_K || nprobe < 1) MM_FAIL(MMISS_ERR_ARG, "%s: Q=%d k=%d nprobe=%d", who, Q, k, nprobe);
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NEED_PARTITION(ix, who);
    const ProbePlan p = plan_probed(ix, Q, k, nprobe);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = p.splits; out[1] = PROBE_SEG; out[2] = p.levels; out[3] = p.qchunk;
    out[4] = (int32_t)std::min<int64_t>(p.bound, INT32_MAX); out[5] = p.share; out[6] = p.NP; out[7] = (Q + p.qchunk - 1) / p.qchunk;
    return MMISS_OK;
}

// mmiss_debug.h: the path a radius call of Q queries would take on the index as it stands, chunk by chunk: the functions
// radius_chunk itself calls, nothing launched, no state changed.
extern "C" int mmiss_dbg_index_radius_plan(mmiss_index* ix, int32_t Q, int32_t filtered, int32_t* out) {
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_radius_plan: null argument");
    if (Q <= 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_radius_plan: Q=%d", Q);
    std::lock_guard<std::mutex> lk(ix->mu);
    for (int i = 0; i < 16; ++i) out[i] = 0;
    const int64_t N = ix->count;
    const int chunks = (Q + RADIUS_CHUNK - 1) / RADIUS_CHUNK;
    out[0] = chunks;
    const int Qc[2] = {std::min<int>(Q, RADIUS_CHUNK), Q - (chunks - 1) * RADIUS_CHUNK};   // the first chunk, the last
    for (int i = 0; i < 2; ++i) {
        int32_t* o = out + 1 + 7 * i;
        o[0] = Qc[i];
        if (N <= 0) continue;   // (an empty index: no pass at all)
        if (sweep_uses_gemm(ix, filtered != 0, Qc[i])) {
            const int64_t nbn = round_up(N, 256) / 256;
            o[1] = 1;
            o[2] = strip_length((int)round_up(Qc[i], 256), nbn, nbn, plan_options());
        } else {
            const DensePlan sp = plan_dense(ix->dim, ix->qelt(), Qc[i], N, false);
            o[3] = sp.nqt; o[4] = sp.slabs; o[5] = sp.tiles_per_block; o[6] = sp.qtiles;
        }
    }
    return MMISS_OK;
}

// mmiss_debug.h: how the dense scans (membership / tagging, assignment, cluster sums) and the kernels behind them would run over
// the index as it stands with n_operands probes / centres / clusters: the functions the calls themselves use, nothing launched, no
// state changed.
extern "C" int mmiss_dbg_index_dense_plan(mmiss_index* ix, int32_t n_operands, int32_t* out) {
    const char* who = "mmiss_dbg_index_dense_plan";
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "%s: null argument", who);
    if (n_operands < 1 || n_operands > ASSIGN_MAX_CENTRES) MM_FAIL(MMISS_ERR_ARG, "%s: n_operands=%d (1 .. %d)", who, n_operands, ASSIGN_MAX_CENTRES);
    std::lock_guard<std::mutex> lk(ix->mu);
    for (int i = 0; i < 40; ++i) out[i] = 0;
    const int64_t N = ix->count;
    auto i32 = [](int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); };
    out[37] = i32(N);
    if (N <= 0) return MMISS_OK;   // (an empty index: no launch at all)
    const DensePlan dp = plan_dense(ix->dim, ix->qelt(), n_operands, N, true);
    out[0] = dp.nqt; out[1] = dp.lds; out[2] = dp.slabs; out[3] = dp.tiles_per_block; out[4] = dp.passes;
    out[5] = dp.tiles_per_block / 4;   // trips of every wave of a full block: tiles tile0 + wave, + 4, ...
    out[6] = 16 * dp.tiles_per_block;  // rows of a block
    const struct { int grid, per_block; } k[7] = {
        {canonical_scan_grid(N), PLAN_CANON_ROWS_PER_BLOCK},  {assign_resolve_grid(N), PLAN_CANON_ROWS_PER_BLOCK},
        {member_count_grid(N), PLAN_POINT_ROWS_PER_BLOCK},    {assign_sizes_grid(N), PLAN_POINT_ROWS_PER_BLOCK},
        {assign_decide_grid(N), PLAN_POINT_ROWS_PER_BLOCK},   {member_from_dist_grid(N), PLAN_POINT_ROWS_PER_BLOCK},
        {member_merge_tags_grid(N), PLAN_POINT_ROWS_PER_BLOCK}};
    for (int i = 0; i < 7; ++i) {
        const int64_t per_trip = (int64_t)k[i].grid * k[i].per_block;
        out[8 + 3 * i] = k[i].grid; out[9 + 3 * i] = i32(per_trip); out[10 + 3 * i] = i32((N + per_trip - 1) / per_trip);
    }
    const ClusterSumsPlan cp = plan_cluster_sums(ix->dim, n_operands, N);
    out[30] = cp.cols; out[31] = cp.chunks; out[32] = cp.rows_per_block; out[33] = cp.slabs; out[34] = cp.lds;
    out[35] = subset_compact_blocks(N); out[36] = PLAN_SUBSET_BLOCK_ROWS;
    return MMISS_OK;
}

// mmiss_debug.h: the plan a query call of this shape would follow on the index as it stands. Host arithmetic only: the functions
// the query path itself calls, nothing launched, no state changed.
extern "C" int mmiss_dbg_index_plan(mmiss_index* ix, int32_t Q, int32_t k, int32_t filtered, int32_t flagged, int32_t* out) {
    if (!ix || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_plan: null argument");
    if (Q <= 0 || k <= 0 || flagged < 0 || flagged > Q) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_plan: Q=%d k=%d flagged=%d", Q, k, flagged);
    std::lock_guard<std::mutex> lk(ix->mu);
    for (int i = 0; i < 24; ++i) out[i] = 0;
    const int64_t N = ix->count;
    const bool filt = filtered != 0;
    QueryPlan p;
    MM_TRY(plan_query(ix, Q, k, filt, p));
    auto i32 = [](int64_t v) { return (int32_t)std::min<int64_t>(v, INT32_MAX); };
    out[0] = p.dense; out[1] = p.dense8; out[2] = p.dense && p.big; out[3] = p.strip_v3; out[4] = p.sample;
    out[5] = p.kp; out[6] = p.pages;
    if (N <= 0) return MMISS_OK;   // (an empty index: no pass at all)
    if (p.dense) {
        out[7] = p.Mq; out[8] = i32(p.Npad); out[9] = i32(p.ns_tiles); out[10] = p.strip;
        const int ng = (int)(p.Ndense / 16);
        out[16] = select_splits(ng, Q);
        out[17] = merge_two_level(p.sample ? 1 : out[16], plan_options());   // (sample form: the last merge reads the one seed list)
        out[23] = select_split_groups(ng, out[16]);
    } else {
        const ScanPlan sp = plan_scan(ix->dim, ix->qelt(), Q, p.kp, N, plan_options());
        out[11] = sp.nqt; out[12] = sp.cap; out[13] = sp.slabs; out[14] = sp.tiles_per_block; out[15] = sp.qtiles;
        out[17] = merge_two_level(sp.slabs, plan_options());
    }
    if (flagged > 0) {
        if (sweep_uses_gemm(ix, filt, flagged)) {
            const int64_t nbn = round_up(N, 256) / 256;
            out[18] = 1;
            out[22] = strip_length((int)round_up(flagged, 256), nbn, nbn, plan_options());
        } else {
            const DensePlan sp = plan_dense(ix->dim, ix->qelt(), flagged, N, false);
            out[19] = sp.nqt; out[20] = sp.slabs; out[21] = sp.tiles_per_block;
        }
    }
    return MMISS_OK;
}

// mmiss_debug.h: the row store as it lies on the device (rows behind count included), to host buffers. Reads only.
extern "C" int mmiss_dbg_index_read_rows(mmiss_index* ix, int64_t row0, int64_t n, void* rows_out, float* inv_out, int64_t* labels_out,
                                         uint64_t* tags_out) {
    if (!ix) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_read_rows: null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_dbg_index_read_rows");
    if (row0 < 0 || n < 0 || row0 > ix->capacity || n > ix->capacity - row0)
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_read_rows: rows [%lld, %lld + %lld) of a capacity of %lld", (long long)row0,
                (long long)row0, (long long)n, (long long)ix->capacity);
    if (n == 0) return MMISS_OK;
    MM_TRY(mmiss_use_device(ix->device));
    MM_HIP(hipStreamSynchronize(ix->stream()));   // (what an earlier call left queued on a caller's stream)
    const size_t row_bytes = (size_t)ix->dim * ix->elt;
    if (rows_out) MM_HIP(hipMemcpy(rows_out, ix->rows.as<char>() + (size_t)row0 * row_bytes, (size_t)n * row_bytes, hipMemcpyDeviceToHost));
    if (inv_out && ix->dtype == MMISS_F8) MM_HIP(hipMemcpy(inv_out, ix->inv.as<float>() + row0, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (labels_out) MM_HIP(hipMemcpy(labels_out, ix->labels_d.as<int64_t>() + row0, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (tags_out) MM_HIP(hipMemcpy(tags_out, ix->tags.as<uint64_t>() + row0, (size_t)n * 8, hipMemcpyDeviceToHost));
    return MMISS_OK;
}

// mmiss_debug.h: upload_queries as a query call runs it, and what it left in qn / qs / eps_q, to host buffers.
extern "C" int mmiss_dbg_index_prep_queries(mmiss_index* ix, const float* queries, int32_t Q, float* qn_out, void* qs_out, float* eps_out) {
    if (!ix || !queries) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_prep_queries: null argument");
    if (Q <= 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_index_prep_queries: Q=%d", Q);
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_dbg_index_prep_queries", &st));
    MM_TRY(upload_queries(ix, st, queries, Q));
    MM_HIP(hipStreamSynchronize(st));
    const size_t D = (size_t)ix->dim, Qpad = (size_t)round_up(Q, 256);
    if (qn_out) MM_HIP(hipMemcpy(qn_out, ix->qn.p, (size_t)Q * D * 4, hipMemcpyDeviceToHost));
    if (qs_out) MM_HIP(hipMemcpy(qs_out, ix->qs.p, Qpad * D * ix->qelt(), hipMemcpyDeviceToHost));
    if (eps_out) MM_HIP(hipMemcpy(eps_out, ix->eps_q.p, (size_t)Q * 4, hipMemcpyDeviceToHost));
    return MMISS_OK;
}

// ================================================================================================ persistence
namespace {
struct IdxHeader {
    char magic[8];
    int32_t version, dim, dtype, reserved;
    int64_t count;
};

// the `n` rows of an index file, read behind its header and labels `lab`, over the index's own buffers (capacity >= n), with
// their labels, inverse norms and tags; any failure leaves rows that no longer match the index's other state
int load_rows(mmiss_index* ix, FILE* f, const char* path, int64_t n, const std::vector<int64_t>& lab, hipStream_t st) {
    const size_t row_bytes = (size_t)ix->dim * ix->elt;
    const int64_t chunk = std::max<int64_t>(1, (64 << 20) / (int64_t)row_bytes);
    std::vector<char> buf((size_t)std::min<int64_t>(chunk, std::max<int64_t>(n, 1)) * row_bytes);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        if (fread(buf.data(), row_bytes, (size_t)nr, f) != (size_t)nr ||
            hipMemcpy(ix->rows.as<char>() + (size_t)r0 * row_bytes, buf.data(), (size_t)nr * row_bytes, hipMemcpyHostToDevice) != hipSuccess)
            MM_FAIL(MMISS_ERR_IO, "%s could not be read to its end", path);
    }
    if (n) MM_HIP(hipMemcpy(ix->labels_d.p, lab.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    // fp8 rows: the file holds the codes only; their inverse norms are a function of the codes (files of round 4 load as they are)
    if (ix->dtype == MMISS_F8 && ix->capacity > 0) {
        MM_HIP(hipMemsetAsync(ix->inv.p, 0, (size_t)ix->capacity * 4, st));
        MM_TRY(launch_f8_inv(ix, 0, n, st));
        MM_HIP(hipStreamSynchronize(st));
    }
    // the file holds no tags (format version 1): every row's tag is 0 after a load
    if (ix->capacity > 0) {
        MM_HIP(hipMemsetAsync(ix->tags.p, 0, (size_t)ix->capacity * 8, st));
        MM_HIP(hipStreamSynchronize(st));
    }
    return MMISS_OK;
}
}  // namespace

extern "C" int mmiss_index_save(mmiss_index* ix, const char* path) {
    if (!ix || !path) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_save: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    MM_NO_PENDING(ix, "mmiss_index_save");
    MM_TRY(mmiss_use_device(ix->device));
    MM_HIP(hipStreamSynchronize(ix->stream()));
    FILE* f = fopen(path, "wb");
    if (!f) MM_FAIL(MMISS_ERR_IO, "cannot open %s for writing", path);
    IdxHeader h{};
    memcpy(h.magic, "MMISSIDX", 8);
    h.version = 1; h.dim = ix->dim; h.dtype = ix->dtype; h.count = ix->count;
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
    if (ok && ix->count) ok = fwrite(ix->labels_h.data(), 8, (size_t)ix->count, f) == (size_t)ix->count;
    const size_t row_bytes = (size_t)ix->dim * ix->elt;
    const int64_t chunk = std::max<int64_t>(1, (64 << 20) / (int64_t)row_bytes);
    std::vector<char> buf((size_t)std::min<int64_t>(chunk, std::max<int64_t>(ix->count, 1)) * row_bytes);
    for (int64_t r0 = 0; ok && r0 < ix->count; r0 += chunk) {
        const int64_t nr = std::min(chunk, ix->count - r0);
        if (hipMemcpy(buf.data(), ix->rows.as<char>() + (size_t)r0 * row_bytes, (size_t)nr * row_bytes,
                      hipMemcpyDeviceToHost) != hipSuccess) { ok = false; break; }
        ok = fwrite(buf.data(), row_bytes, (size_t)nr, f) == (size_t)nr;
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) MM_FAIL(MMISS_ERR_IO, "write to %s failed", path);
    return MMISS_OK;
}

extern "C" int mmiss_index_load(mmiss_index* ix, const char* path) {
    if (!ix || !path) MM_FAIL(MMISS_ERR_ARG, "mmiss_index_load: null argument");
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = nullptr;
    MM_TRY(enter(ix, "mmiss_index_load", &st));
    // the rows are overwritten by blocking copies that do not run on `st`: a query with device outputs may still be queued on a
    // caller's stream (async_pending) and reads them
    MM_HIP(hipStreamSynchronize(st));
    FILE* f = fopen(path, "rb");
    if (!f) MM_FAIL(MMISS_ERR_IO, "cannot open %s", path);
    IdxHeader h{};
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "MMISSIDX", 8) != 0 || h.version != 1) {
        fclose(f);
        MM_FAIL(MMISS_ERR_IO, "%s is not an mmiss index file", path);
    }
    if (h.dim != ix->dim || h.dtype != ix->dtype || h.count < 0) {
        fclose(f);
        MM_FAIL(MMISS_ERR_ARG, "%s holds dim %d dtype %d; this index is dim %d dtype %d", path, h.dim, h.dtype, ix->dim,
                ix->dtype);
    }
    const size_t row_bytes = (size_t)ix->dim * ix->elt;
    {   // a truncated file is refused BEFORE anything of the index is overwritten: the header's count against the file's length
        const long at = ftell(f);
        long end = -1;
        if (at >= 0 && fseek(f, 0, SEEK_END) == 0) end = ftell(f);
        if (at < 0 || end < 0 || fseek(f, at, SEEK_SET) != 0) { fclose(f); MM_FAIL(MMISS_ERR_IO, "cannot seek in %s", path); }
        if ((uint64_t)h.count > (uint64_t)(end - at) / (8 + row_bytes)) {
            fclose(f);
            MM_FAIL(MMISS_ERR_IO, "%s is truncated or corrupt (%ld bytes behind the header, %lld rows need %llu); the index is unchanged",
                    path, end - at, (long long)h.count, (unsigned long long)((uint64_t)h.count * (8 + row_bytes)));
        }
    }
    std::vector<int64_t> lab((size_t)h.count);
    bool ok = h.count == 0 || fread(lab.data(), 8, (size_t)h.count, f) == (size_t)h.count;
    for (int64_t i = 1; ok && i < h.count; ++i) ok = lab[i] > lab[i - 1];
    if (!ok) { fclose(f); MM_FAIL(MMISS_ERR_IO, "%s: labels unreadable or not strictly increasing; the index is unchanged", path); }
    int rc = index_reserve(ix, h.count, st);
    if (rc != MMISS_OK) { fclose(f); return rc; }
    drop_partition(ix);   // (the rows are replaced; the file holds no partition)
    rc = load_rows(ix, f, path, h.count, lab, st);
    fclose(f);
    if (rc != MMISS_OK) {
        // part of the rows already overwritten: old labels / inverse norms no longer describe what the buffer holds, so the
        // index is left EMPTY rather than inconsistent
        const std::string why = mmiss_last_error();
        (void)reset_rows(ix, st);
        MM_FAIL(rc, "%s; the index was cleared", why.c_str());
    }
    ix->tags_h.assign((size_t)h.count, 0);
    ix->groups_h.assign((size_t)h.count, -1); ix->group_hwm = 0; ix->groups_dirty = true;   // (the file holds no groups either)
    ix->labels_h.swap(lab);
    ix->count = h.count;
    return MMISS_OK;
}

// ================================================================================================ glue kernels
extern "C" int mmiss_blend(int device, void* hip_stream, const float* img, const float* txt, double w, int32_t Q,
                           int32_t dim, float* out) {
    if (!img || !txt || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_blend: null argument");
    if (Q < 0 || dim <= 0 || dim % 64) MM_FAIL(MMISS_ERR_ARG, "mmiss_blend: Q=%d dim=%d (dim must be a multiple of 64)", Q, dim);
    if (Q == 0) return MMISS_OK;
    MM_TRY(mmiss_use_device(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const size_t bytes = (size_t)Q * dim * 4;
    DevBuf bi, bt, bo;
    const float *di = img, *dt = txt;
    float* dout = out;
    if (!mmiss_is_device_ptr(img)) { MM_TRY(bi.alloc(bytes)); MM_HIP(hipMemcpyAsync(bi.p, img, bytes, hipMemcpyHostToDevice, st)); di = bi.as<float>(); }
    if (!mmiss_is_device_ptr(txt)) { MM_TRY(bt.alloc(bytes)); MM_HIP(hipMemcpyAsync(bt.p, txt, bytes, hipMemcpyHostToDevice, st)); dt = bt.as<float>(); }
    const bool out_dev = mmiss_is_device_ptr(out);
    if (!out_dev) { MM_TRY(bo.alloc(bytes)); dout = bo.as<float>(); }
    {
        MM_PROF("blend", st, 12.0 * Q * dim, 3.0 * bytes);
        hipLaunchKernelGGL(blend_kernel, dim3((Q + 3) / 4), dim3(256), 0, st, di, dt, (float)w, (float)(1.0 - w), Q, dim, dout);
        MM_HIP(hipGetLastError());
    }
    if (!out_dev) MM_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
    if (!out_dev || bi.p || bt.p) MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

// one merge level: S lists of k per query -> one list of k (S * k <= 8192 entries sorted in LDS)
static int launch_shard_merge(hipStream_t st, const float* dd, const int64_t* dl, int S, int Q, int k, float* dod,
                              int64_t* dol, int32_t* doc) {
    int npow = 1;
    while (npow < S * k) npow <<= 1;
    const int lds = npow * 12 + 16;
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&shard_merge_kernel), lds));
    MM_PROF("shard_merge", st, 0.0, (double)S * Q * k * 12);
    hipLaunchKernelGGL(shard_merge_kernel, dim3(Q), dim3(256), lds, st, dd, dl, S, Q, k, dod, dol, doc);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

extern "C" int mmiss_merge_topk(int device, void* hip_stream, const float* dist, const int64_t* labels, int32_t S,
                                int32_t Q, int32_t k, float* out_dist, int64_t* out_labels, int32_t* out_count) {
    if (!dist || !labels || !out_dist || !out_labels) MM_FAIL(MMISS_ERR_ARG, "mmiss_merge_topk: null argument");
    if (S <= 0 || Q < 0 || k <= 0 || k > 4096)
        MM_FAIL(MMISS_ERR_ARG, "mmiss_merge_topk: S=%d Q=%d k=%d (need S > 0, 0 < k <= 4096)", S, Q, k);
    if (Q == 0) return MMISS_OK;
    MM_TRY(mmiss_use_device(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const size_t n_in = (size_t)S * Q * k, n_out = (size_t)Q * k;
    DevBuf bd, bl, bod, bol, boc, td[2], tl[2];
    const float* dd = dist; const int64_t* dl = labels;
    float* dod = out_dist; int64_t* dol = out_labels; int32_t* doc = out_count;
    if (!mmiss_is_device_ptr(dist)) { MM_TRY(bd.alloc(n_in * 4)); MM_HIP(hipMemcpyAsync(bd.p, dist, n_in * 4, hipMemcpyHostToDevice, st)); dd = bd.as<float>(); }
    if (!mmiss_is_device_ptr(labels)) { MM_TRY(bl.alloc(n_in * 8)); MM_HIP(hipMemcpyAsync(bl.p, labels, n_in * 8, hipMemcpyHostToDevice, st)); dl = bl.as<int64_t>(); }
    const bool out_dev = mmiss_is_device_ptr(out_dist);
    if (!out_dev) {
        MM_TRY(bod.alloc(n_out * 4)); MM_TRY(bol.alloc(n_out * 8)); MM_TRY(boc.alloc((size_t)Q * 4));
        dod = bod.as<float>(); dol = bol.as<int64_t>(); doc = boc.as<int32_t>();
    }
    // The reference's "All" search asks for 1000 hits (main.py:757): 8 shards x 1000 = 8000 entries sort in one 96 KB LDS
    // pass. Beyond 8192 entries the lists are merged in groups of G = 8192 / k lists per level (a top-k of top-k's is
    // the top-k), each level S -> ceil(S / G) lists, until one is left.
    const int G = 8192 / k;  // >= 2 because k <= 4096
    int cur_S = S, flip = 0;
    while (cur_S > G) {
        const int nxt = (cur_S + G - 1) / G;
        MM_TRY(td[flip].ensure((size_t)nxt * n_out * 4));
        MM_TRY(tl[flip].ensure((size_t)nxt * n_out * 8));
        for (int g = 0; g < nxt; ++g) {
            const int s0 = g * G, sn = std::min(G, cur_S - s0);
            MM_TRY(launch_shard_merge(st, dd + (size_t)s0 * n_out, dl + (size_t)s0 * n_out, sn, Q, k,
                                      td[flip].as<float>() + (size_t)g * n_out, tl[flip].as<int64_t>() + (size_t)g * n_out, nullptr));
        }
        dd = td[flip].as<float>(); dl = tl[flip].as<int64_t>();
        cur_S = nxt;
        flip ^= 1;
    }
    MM_TRY(launch_shard_merge(st, dd, dl, cur_S, Q, k, dod, dol, doc));
    if (!out_dev) {
        MM_HIP(hipMemcpyAsync(out_dist, dod, n_out * 4, hipMemcpyDeviceToHost, st));
        MM_HIP(hipMemcpyAsync(out_labels, dol, n_out * 8, hipMemcpyDeviceToHost, st));
        if (out_count) MM_HIP(hipMemcpyAsync(out_count, doc, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    }
    if (!out_dev || bd.p || bl.p || td[0].p || td[1].p) MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}
