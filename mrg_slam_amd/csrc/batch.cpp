// csrc/batch.cpp — mrgfe_batch: the candidate batch behind loop closure, the node (mrgfe_node_*), the loop detector and the keyframe store.  A PairBook
// says which pairs there are; the method's engine runs their rounds (NdtEngine for the NDTs, GicpBatch over one GicpEngine per target for the LM GICPs and
// ICP_HIP); the fitness passes — overlapped with the rounds for NDT (FitOverlap) — fill in getFitnessScore; one writer makes the records.  Also here: the
// batch's keyframe store, its asynchronous worker, and mrgfe_batch_clear_pairs (the pairs go, the targets and what was built for them stay).  Entry
// points follow the rules of api.cpp: codes and a thread-local message, no exception crosses.
#include <atomic>
#include <cfloat>
#include <condition_variable>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <mutex>
#include <thread>

#include "api_internal.h"
#include "fit_select.h"
#include "ndt_derivatives.h"
#include "resident_cache.h"

using namespace mrgfe;

struct mrgfe_batch {
    explicit mrgfe_batch(mrgfe_ctx* c) : ctx(c), book(c) {}
    mrgfe_ctx*       ctx;
    mrgfe_reg_params params;
    // Members go in reverse order of declaration: the helper contexts stand before the engines and grids that were filled on their streams, so they go after
    // them (every thread that used one has been joined by then: FitOverlap, and mrgfe_batch_destroy for the asynchronous worker).
    CtxPtr              early_ctx;          // lowest-priority context of the early fitness pass (mrgfe_batch_align)
    std::vector<CtxPtr> fit_ctxs;           // helper contexts (own stream and workspaces each): the grids are built on them by extra host
                                            // thread while the alignment rounds run on the batch's context
    PairBook            book;         // the targets, pairs and guesses of the batch, and the device copies of its host-supplied clouds: every method reads it
    std::unique_ptr<NdtEngine> ndt;   // NDT_HIP, PCL_NDT_HIP only: the grids and optimisers over the book (declared after it, so destroyed before it)
    std::vector<std::unique_ptr<GicpEngine>> gicp;  // GICP_HIP: one engine per target (its covariances and correspondence grid are computed once)
    std::vector<float>  final_rm;     // row-major final transformation of every pair (P * 16), filled after the rounds of every method
    std::unique_ptr<GicpBatch> gicp_batch;
    std::vector<GicpBatchPair> gicp_pairs;  // per-pair device buffers, kept between align calls
    std::vector<NnGrid> fit_grids;  // getFitnessScore grids, one per target; device buffers kept between align calls
    std::vector<std::unique_ptr<NnGridSet>> fit_sets;  // ... which are views into these when the grids were built a chunk of targets at a time
    // mrgfe_batch_clear_pairs keeps the targets: their fitness grids stay good (fit_valid, per target), and so do the sets the valid grids are views
    // into (the first fit_sets_used of fit_sets: a later build takes the sets behind them).  mrgfe_batch_clear forgets both.
    std::vector<char>   fit_valid;
    size_t              fit_sets_used = 0;
    // keyframe store (mrgfe_batch_add_pair_keyed): packed clouds and GICP covariances by caller-chosen key, resident across clears.  An era of the
    // cache is one batch: what was named since the last clear / clear_pairs is in use.
    struct Keyframe {
        DevBuf   cloud, cov;  // (no cloud: an entry of mrgfe_batch_add_pair_from_store, whose cloud a map store or a node member's replica owns)
        uint32_t n = 0;
        int      cov_k = 0;   // k_correspondences the covariances were computed with; 0: none yet
        size_t   bytes() const { return cloud.cap + cov.cap; }
    };
    using Store = ResidentCache<uint64_t, Keyframe>;
    Store store;
    std::vector<uint64_t> pair_key;  // per pair; 0: not from the store
    FitStats   fit_total;             // getFitnessScore passes of the last align(), all waves added up
    FitSelectStats select_stats;      // the last mrgfe_batch_align_best
    std::vector<double> fit_lo, fit_hi;  // per pair: the fitness interval of the last mrgfe_batch_align_best (mrgfe_dbg_batch_fit_bounds)
    // batch_align_bounds .. batch_align_finish: the selection between its two stages.  While `run` is pending nothing else may use the batch's context
    // (FitSelectRun, nn_grid.h): both stages of mrgfe_batch_align_best run under one hold of the context lock, and a node member's batch is reached
    // through its node alone.
    struct Select {
        FitSelectRun     run;
        std::vector<int> job_pair;  // the pair of every fitness job of the run
        std::chrono::steady_clock::time_point t_start;  // mrgfe_batch_timing: the align that ends with the second stage
    } select;
    std::unique_ptr<NdtSnapshotPort> port;  // early fitness passes (mrgfe_batch_align)
    Event      uploads_done;  // recorded on ctx->stream before helper streams read the batch's clouds (upload_cloud is stream-ordered only)
    // mrgfe_batch_timing: the reference's per-candidate time (loop_detector.cpp:22-34): from the clear that starts queueing a batch to its records
    std::chrono::steady_clock::time_point t_queue;
    bool     t_queue_set = false;
    double   last_us = 0.0, total_us = 0.0;
    int64_t  last_pairs = 0, total_pairs = 0;
    // mrgfe_batch_align_async / mrgfe_batch_wait: a worker thread of the batch's own runs mrgfe_batch_align while the caller queues the next batch
    // on another object.  It takes the context lock BEFORE the async call returns, so every other call on this batch simply waits for the align.
    struct Async {
        std::thread th;
        std::mutex  mu;
        std::condition_variable cv;
        int    state = 0;  // 0 idle, 1 posted, 2 running (context lock held), 3 finished and not yet waited for
        bool   quit = false;
        double fitness_max_range = -1.0;
        mrgfe_pair_result* results = nullptr;
        // mrgfe_batch_align_best_async: the selection arguments (`group` copied at the call), else best = false
        bool   best = false;
        double score_cap = DBL_MAX;
        std::vector<int32_t> group;
        int    n_groups = 0;
        int32_t *fit_state = nullptr, *best_out = nullptr;
        double*  best_score = nullptr;
        int    status = MRGFE_OK;
        std::string error;
    };
    std::unique_ptr<Async> async;
};

// The store's entry for keyframe `key` with `n` points, for a pair that `fn` is adding: the resident one, or a fresh one after room was made for it — with `own_cloud`
// its packed cloud, uploaded from `xyzi`; without, for the covariances alone.  An entry that does not fit (another size, or no cloud where one is to be owned) is
// replaced, unless this batch already uses it.  The context is locked and bound.
static int store_entry(mrgfe_batch* b, const char* fn, uint64_t key, size_t n, bool own_cloud, const float* xyzi, size_t stride, mrgfe_batch::Store::Entry** out)
{
    mrgfe_batch::Store::Entry* e = b->store.find(key);
    if (e && e->data.n == n && (e->data.cloud.p || !own_cloud)) { *out = e; return MRGFE_OK; }
    if (own_cloud && n && !xyzi) { set_error("%s: key %llu is not in the store (or has another size) and no cloud was given", fn, static_cast<unsigned long long>(key)); return MRGFE_ERR_INVALID; }
    if (e && b->store.in_use(*e)) { set_error("%s: key %llu is already used in this batch with %u points", fn, static_cast<unsigned long long>(key), e->data.n); return MRGFE_ERR_INVALID; }
    b->store.erase(key);  // (the entry that does not fit, if there is one)
    b->store.make_room((own_cloud ? n * 16 : 0) + (keeps_covariances(b->params) ? n * 48 : 0));
    if (!(e = b->store.find_or_insert(key))) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
    e->data.n = static_cast<uint32_t>(n);
    if (own_cloud) {
        // (ICP_HIP keeps the cloud alone and the entry never grows: mrgfe_batch_store_bytes counts 16 bytes per point, no allocation headroom)
        DevBuf& c = e->data.cloud;
        int st = b->params.method == MRGFE_ICP_HIP ? c.ensure_exact(std::max<size_t>(n, 1) * 16) : c.ensure(std::max<size_t>(n, 1) * 16);
        if (st == MRGFE_OK && n) st = upload_cloud(b->ctx, xyzi, n, stride, c.p);
        if (st != MRGFE_OK) { b->store.erase(key); return st; }
    }
    *out = e;
    return MRGFE_OK;
}

// pair (target, the packed device cloud `p`) of keyframe `key`; its store entry `e` (null: nothing is kept for it) is named by the batch
static int add_stored_pair(mrgfe_batch* b, int target, uint64_t key, mrgfe_batch::Store::Entry* e, const void* p, size_t n, const float guess[16])
{
    if (e) b->store.touch(*e);
    float g[16];
    col2row(guess, g);
    const int pair = b->book.add_pair_device(target, p, n, g);
    if (pair >= 0 && e) {
        if (b->pair_key.size() <= static_cast<size_t>(pair)) b->pair_key.resize(pair + 1, 0);
        b->pair_key[pair] = key;
    }
    return pair;
}

extern "C" {

// ---- batch ------------------------------------------------------------------------------------------------------
int mrgfe_batch_create(mrgfe_ctx* ctx, const mrgfe_reg_params* params, mrgfe_batch** out)
{
    return abi_guard("mrgfe_batch_create", [&]() -> int {
        if (!ctx || !out) { set_error("mrgfe_batch_create: NULL argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        MRGFE_TRY(check_params(params));
        if (is_pcl_gicp(params->method) && !ctx->bfgs_batches.load(std::memory_order_relaxed)) {  // (mrgfe_ctx_set_bfgs_batches opens the door)
            set_error("mrgfe_batch_create: PCL_GICP_HIP and PCL_GICP_OMP_HIP are offered for single registrations only");
            return MRGFE_ERR_INVALID;
        }
        std::unique_ptr<mrgfe_batch> b(new (std::nothrow) mrgfe_batch(ctx));
        if (!b) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        b->params = *params;
        if (is_ndt(params->method)) b->ndt = std::make_unique<NdtEngine>(ctx, ndt_params_from(*params), &b->book);
        b->store.set_cap(mrgfe_batch::Store::cap_from_env(size_t(16384) << 20));
        *out = b.release();
        return MRGFE_OK;
    });
}
static void batch_async_main(mrgfe_batch* b)
{
    mrgfe_batch::Async& a = *b->async;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(a.mu);
            a.cv.wait(lk, [&] { return a.state == 1 || a.quit; });
            if (a.quit) return;
        }
        int st;
        std::string err;
        {
            MRGFE_LOCK(b->ctx);
            {
                std::lock_guard<std::mutex> lk(a.mu);
                a.state = 2;
            }
            a.cv.notify_all();
            // (an exception becomes an error code for the waiter, never std::terminate)
            st = abi_guard("mrgfe_batch_align_async", [&] {
                if (!a.best) return mrgfe_batch_align(b, a.fitness_max_range, a.results);
                return mrgfe_batch_align_best(b, a.fitness_max_range, a.score_cap, a.group.data(), a.n_groups, a.results, a.fit_state, a.best_out, a.best_score);
            });
            if (st != MRGFE_OK) err = mrgfe_last_error();
        }
        {
            std::lock_guard<std::mutex> lk(a.mu);
            a.status = st;
            a.error = err;
            a.state = 3;
        }
        a.cv.notify_all();
    }
}

// Hand an align to the batch's worker (started on first use): `fill` writes the arguments into the idle Async record.  Returns once the worker holds the
// context lock, so later calls on this batch queue up behind the align.
extern "C++" template <class Fill>
static int batch_post_async(mrgfe_batch* b, const char* fn, Fill fill)
{
    if (!b->async) {
        b->async.reset(new (std::nothrow) mrgfe_batch::Async());
        if (!b->async) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        const int st = abi_guard(fn, [&] { b->async->th = std::thread(batch_async_main, b); return MRGFE_OK; });
        if (st != MRGFE_OK) { b->async.reset(); return st; }
    }
    mrgfe_batch::Async& a = *b->async;
    std::unique_lock<std::mutex> lk(a.mu);
    if (a.state != 0) { set_error("%s: an align of this batch is %s: call mrgfe_batch_wait first", fn, a.state == 3 ? "finished and not yet waited for" : "in flight"); return MRGFE_ERR_STATE; }
    fill(a);
    a.state = 1;
    a.cv.notify_all();
    a.cv.wait(lk, [&] { return a.state >= 2; });  // the worker holds the context lock now: later calls on this batch queue up behind the align
    return MRGFE_OK;
}

int mrgfe_batch_align_async(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results)
{
    return abi_guard("mrgfe_batch_align_async", [&]() -> int {
        if (!b || !results) { set_error("mrgfe_batch_align_async: NULL argument"); return MRGFE_ERR_INVALID; }
        return batch_post_async(b, "mrgfe_batch_align_async", [&](mrgfe_batch::Async& a) {
            a.best = false;
            a.fitness_max_range = fitness_max_range;
            a.results = results;
        });
    });
}

static int check_best_args(const mrgfe_batch* b, double fitness_max_range, double score_cap, const int32_t* group, int n_groups, const mrgfe_pair_result* results,
                           const int32_t* best, const double* best_score);

int mrgfe_batch_align_best_async(mrgfe_batch* b, double fitness_max_range, double score_cap, const int32_t* group, int n_groups, mrgfe_pair_result* results, int32_t* fit_state,
                                 int32_t* best, double* best_score)
{
    return abi_guard("mrgfe_batch_align_best_async", [&]() -> int {
        if (!b) { set_error("mrgfe_batch_align_best: NULL argument"); return MRGFE_ERR_INVALID; }
        // A running align holds the context lock the argument check needs (the pair list must not move under it): refuse here rather than wait for it.
        // (Only this thread can start an align between this look and the post below: a batch has one caller at a time.)
        if (b->async) {
            mrgfe_batch::Async& a = *b->async;
            std::lock_guard<std::mutex> lk(a.mu);
            if (a.state != 0) { set_error("mrgfe_batch_align_best_async: an align of this batch is %s: call mrgfe_batch_wait first", a.state == 3 ? "finished and not yet waited for" : "in flight"); return MRGFE_ERR_STATE; }
        }
        int P;
        {
            MRGFE_LOCK(b->ctx);
            MRGFE_TRY(check_best_args(b, fitness_max_range, score_cap, group, n_groups, results, best, best_score));
            P = b->book.n_pairs();
        }
        return batch_post_async(b, "mrgfe_batch_align_best_async", [&](mrgfe_batch::Async& a) {
            a.best = true;
            a.fitness_max_range = fitness_max_range;
            a.score_cap = score_cap;
            a.group.assign(group, group + (group ? P : 0));
            a.n_groups = n_groups;
            a.results = results;
            a.fit_state = fit_state;
            a.best_out = best;
            a.best_score = best_score;
        });
    });
}

int mrgfe_batch_wait(mrgfe_batch* b)
{
    if (!b) { set_error("mrgfe_batch_wait: NULL batch"); return MRGFE_ERR_INVALID; }
    if (!b->async) { set_error("mrgfe_batch_wait: no asynchronous align was started"); return MRGFE_ERR_STATE; }
    mrgfe_batch::Async& a = *b->async;
    std::unique_lock<std::mutex> lk(a.mu);
    if (a.state == 0) { set_error("mrgfe_batch_wait: no asynchronous align was started"); return MRGFE_ERR_STATE; }
    a.cv.wait(lk, [&] { return a.state == 3; });
    a.state = 0;
    if (a.status != MRGFE_OK) set_error("%s", a.error.c_str());
    return a.status;
}

void mrgfe_batch_destroy(mrgfe_batch* b)
{
    if (!b) return;
    if (b->async) {  // before the context lock below: a running align holds it
        mrgfe_batch::Async& a = *b->async;
        {
            std::unique_lock<std::mutex> lk(a.mu);
            a.cv.wait(lk, [&] { return a.state == 0 || a.state == 3; });
            a.quit = true;
        }
        a.cv.notify_all();
        if (a.th.joinable()) a.th.join();
    }
    MRGFE_LOCK(b->ctx);
    (void)b->ctx->bind();
    delete b;
}
int mrgfe_batch_clear(mrgfe_batch* b)
{
    if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    b->book.clear();
    if (b->ndt) b->ndt->clear();
    b->gicp.clear();  // their cached target state belongs to the clouds just forgotten
    b->fit_valid.clear();
    b->fit_sets_used = 0;
    b->pair_key.clear();
    b->store.next_era();  // stored keyframes stay; none is referenced by the (now empty) batch
    b->t_queue = std::chrono::steady_clock::now();  // mrgfe_batch_timing: the next align's time starts where its queueing starts
    b->t_queue_set = true;
    return MRGFE_OK;
}
int mrgfe_batch_clear_pairs(mrgfe_batch* b)
{
    if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    // the targets, the engines' state for them (NdtEngine's grids, one GicpEngine per target, the fitness grids) and the book's uploads stay
    b->book.clear_pairs();
    b->pair_key.clear();
    b->store.next_era();
    b->t_queue = std::chrono::steady_clock::now();
    b->t_queue_set = true;
    return MRGFE_OK;
}
int mrgfe_batch_add_target(mrgfe_batch* b, const float* xyzi, size_t n, size_t stride)
{
    return abi_guard("mrgfe_batch_add_target", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_batch_add_target"));
        if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(b->ctx);
        return b->book.add_target_host(xyzi, n, stride);
    });
}
int mrgfe_batch_add_target_device(mrgfe_batch* b, const void* d, size_t n)
{
    return abi_guard("mrgfe_batch_add_target_device", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_batch_add_target_device"));
        if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(b->ctx);
        return b->book.add_target_device(d, n);
    });
}
int mrgfe_batch_add_pair(mrgfe_batch* b, int target, const float* xyzi, size_t n, size_t stride, const float guess[16])
{
    return abi_guard("mrgfe_batch_add_pair", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_batch_add_pair"));
        if (!b || !guess) { set_error("NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(b->ctx);
        float g[16];
        col2row(guess, g);
        return b->book.add_pair_host(target, xyzi, n, stride, g);
    });
}
int mrgfe_batch_add_pair_device(mrgfe_batch* b, int target, const void* d, size_t n, const float guess[16])
{
    return abi_guard("mrgfe_batch_add_pair_device", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_batch_add_pair_device"));
        if (!b || !guess) { set_error("NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(b->ctx);
        float g[16];
        col2row(guess, g);
        return b->book.add_pair_device(target, d, n, g);
    });
}
int mrgfe_batch_add_device(mrgfe_batch* b, int n_targets, const void* const* d_targets, const size_t* target_points, int n_pairs, const int32_t* pair_target,
                           const void* const* d_sources, const size_t* source_points, const float* guesses)
{
    return abi_guard("mrgfe_batch_add_device", [&]() -> int {
        if (!b || n_targets < 0 || n_pairs < 0 || (n_targets && (!d_targets || !target_points)) || (n_pairs && (!pair_target || !d_sources || !source_points || !guesses))) {
            set_error("mrgfe_batch_add_device: bad argument");
            return MRGFE_ERR_INVALID;
        }
        MRGFE_LOCK(b->ctx);
        const int t0 = b->book.n_targets(), p0 = b->book.n_pairs();
        for (int i = 0; i < n_pairs; ++i)
            if (pair_target[i] < 0 || pair_target[i] >= n_targets) { set_error("mrgfe_batch_add_device: pair %d names target %d of %d", i, pair_target[i], n_targets); return MRGFE_ERR_INVALID; }
        for (int i = 0; i < n_targets; ++i) {
            const int t = b->book.add_target_device(d_targets[i], target_points[i]);
            if (t < 0) return t;
        }
        for (int i = 0; i < n_pairs; ++i) {
            float g[16];
            col2row(guesses + size_t(i) * 16, g);
            const int pi = b->book.add_pair_device(t0 + pair_target[i], d_sources[i], source_points[i], g);
            if (pi < 0) return pi;
        }
        return p0;
    });
}
int mrgfe_batch_add_pair_keyed(mrgfe_batch* b, int target, uint64_t key, const float* xyzi, size_t n, size_t stride, const float guess[16])
{
    return abi_guard("mrgfe_batch_add_pair_keyed", [&]() -> int {
        MRGFE_TRY(check_count(n, "mrgfe_batch_add_pair_keyed"));
        if (!b || !guess) { set_error("NULL argument"); return MRGFE_ERR_INVALID; }
        if (key == 0) return mrgfe_batch_add_pair(b, target, xyzi, n, stride, guess);
        MRGFE_LOCK(b->ctx);
        MRGFE_TRY(b->ctx->bind());
        if (n > 0x7fffffffu) { set_error("cloud too large"); return MRGFE_ERR_INVALID; }
        mrgfe_batch::Store::Entry* e = nullptr;
        MRGFE_TRY(store_entry(b, "mrgfe_batch_add_pair_keyed", key, n, true, xyzi, stride, &e));
        return add_stored_pair(b, target, key, e, e->data.cloud.p, n, guess);
    });
}
int mrgfe_batch_has_cloud(const mrgfe_batch* b, uint64_t key, size_t* n)
{
    if (!b || key == 0) return 0;
    MRGFE_LOCK(b->ctx);
    const mrgfe_batch::Store::Entry* e = b->store.find(key);
    if (!e || !e->data.cloud.p) return 0;  // (no cloud: an entry of mrgfe_batch_add_pair_from_store)
    if (n) *n = e->data.n;
    return 1;
}
size_t mrgfe_batch_store_bytes(const mrgfe_batch* b)
{
    if (!b) return 0;
    MRGFE_LOCK(b->ctx);
    return b->store.bytes();
}
int mrgfe_batch_forget(mrgfe_batch* b, uint64_t key)
{
    if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    MRGFE_TRY(b->ctx->bind());
    if (!b->pair_key.empty())  // (no keyed pair: the batch reads nothing of the store)
        for (auto& kv : b->store)
            if ((key == 0 || kv.first == key) && b->store.in_use(kv.second)) { set_error("mrgfe_batch_forget: key %llu is used by the current batch (clear it first)", static_cast<unsigned long long>(kv.first)); return MRGFE_ERR_STATE; }
    if (key == 0) b->store.clear();
    else          b->store.erase(key);
    return MRGFE_OK;
}
// (api_internal.h) Keyframe `key` of a map store: looked up, and the store's stream waited for (mrgfe_map_store_add uploads asynchronously), under the store's
// lock ALONE — it is released before the caller takes the batch's or the node's lock, so no thread ever holds two of them.
extern "C++" int map_store_lookup(const char* fn, mrgfe_map_store* s, uint64_t key, const float4** p, size_t* n)
{
    MRGFE_LOCK(s->ctx);
    MRGFE_TRY(s->ctx->bind());
    auto it = s->clouds.find(key);
    if (it == s->clouds.end()) { set_error("%s: keyframe %llu is not in the store", fn, static_cast<unsigned long long>(key)); return MRGFE_ERR_INVALID; }
    MRGFE_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
    *p = it->second.p;
    *n = it->second.n;
    return MRGFE_OK;
}
// ... for a batch, which reads the store's memory in place: on the same device
static int store_lookup(const char* fn, const mrgfe_batch* b, mrgfe_map_store* s, uint64_t key, const float4** p, size_t* n)
{
    if (s->ctx->device != b->ctx->device) { set_error("%s: the store is on device %d, the batch on device %d", fn, s->ctx->device, b->ctx->device); return MRGFE_ERR_INVALID; }
    return map_store_lookup(fn, s, key, p, n);
}
int mrgfe_batch_add_target_from_store(mrgfe_batch* b, mrgfe_map_store* s, uint64_t key)
{
    static const char* fn = "mrgfe_batch_add_target_from_store";
    return abi_guard(fn, [&]() -> int {
        if (!b || !s) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        const float4* p = nullptr;
        size_t n = 0;
        MRGFE_TRY(store_lookup(fn, b, s, key, &p, &n));
        MRGFE_LOCK(b->ctx);
        return b->book.add_target_device(p, n);
    });
}
// A pair whose source is the packed device cloud `p` of keyframe `key`: for the methods that keep covariances they are cached in the batch's store under the
// key, next to no cloud (its owner has it: a map store, or a node member's replica of one).  The batch's lock is held.
static int add_pair_device_keyed(mrgfe_batch* b, const char* fn, int target, uint64_t key, const void* p, size_t n, const float guess[16])
{
    MRGFE_TRY(b->ctx->bind());
    if (target < 0 || target >= b->book.n_targets()) { set_error("%s: target index %d out of range", fn, target); return MRGFE_ERR_INVALID; }
    mrgfe_batch::Store::Entry* e = nullptr;
    if (keeps_covariances(b->params)) MRGFE_TRY(store_entry(b, fn, key, n, false, nullptr, 0, &e));
    return add_stored_pair(b, target, key, e, p, n, guess);
}
int mrgfe_batch_add_pair_from_store(mrgfe_batch* b, int target, mrgfe_map_store* s, uint64_t key, const float guess[16])
{
    static const char* fn = "mrgfe_batch_add_pair_from_store";
    return abi_guard(fn, [&]() -> int {
        if (!b || !s || !guess) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        const float4* p = nullptr;
        size_t n = 0;
        MRGFE_TRY(store_lookup(fn, b, s, key, &p, &n));
        MRGFE_LOCK(b->ctx);
        return add_pair_device_keyed(b, fn, target, key, p, n, guess);
    });
}
int mrgfe_batch_set_guess(mrgfe_batch* b, int pair, const float guess[16])
{
    if (!b || !guess) { set_error("NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    float g[16];
    col2row(guess, g);
    return b->book.set_guess(pair, g);
}
int mrgfe_batch_build_targets(mrgfe_batch* b)
{
    if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    if (!is_ndt(b->params.method)) return MRGFE_OK;  // GICP variants and ICP: target covariances and grids are built by the first align
    TraceRange tr("mrgfe set_target (batch)");
    return b->ndt->build_targets();
}
int mrgfe_batch_num_pairs(const mrgfe_batch* b) { return b ? b->book.n_pairs() : 0; }

// `sel_group` (mrgfe_batch_align_best's group per pair, or null): the fitness passes stop after the bound stage and leave b->select pending
static int batch_align_impl(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results, const int32_t* sel_group = nullptr);

static int batch_align_timed(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results);

int mrgfe_batch_align(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results)
{
    return abi_guard("mrgfe_batch_align", [&]() -> int {
        if (!b || !results) { set_error("mrgfe_batch_align: NULL argument"); return MRGFE_ERR_INVALID; }
        return batch_align_timed(b, fitness_max_range, results);
    });
}

// the argument checks of mrgfe_batch_align_best (and of its _async form, in the calling thread); the context lock is held
static int check_best_args(const mrgfe_batch* b, double fitness_max_range, double score_cap, const int32_t* group, int n_groups, const mrgfe_pair_result* results,
                           const int32_t* best, const double* best_score)
{
    if (!b || !results || n_groups < 0 || (n_groups > 0 && (!best || !best_score))) { set_error("mrgfe_batch_align_best: NULL argument"); return MRGFE_ERR_INVALID; }
    const int P = b->book.n_pairs();
    if (P > 0 && !group) { set_error("mrgfe_batch_align_best: NULL group"); return MRGFE_ERR_INVALID; }
    if (!(fitness_max_range >= 0) || std::isnan(score_cap)) { set_error("mrgfe_batch_align_best: fitness_max_range must be >= 0 and score_cap a number"); return MRGFE_ERR_INVALID; }
    for (int i = 0; i < P; ++i)
        if (group[i] < -1 || group[i] >= n_groups) { set_error("mrgfe_batch_align_best: group[%d] = %d is not -1 or in [0, %d)", i, group[i], n_groups); return MRGFE_ERR_INVALID; }
    return MRGFE_OK;
}

int mrgfe_batch_align_best(mrgfe_batch* b, double fitness_max_range, double score_cap, const int32_t* group, int n_groups, mrgfe_pair_result* results, int32_t* fit_state,
                           int32_t* best, double* best_score)
{
    return abi_guard("mrgfe_batch_align_best", [&]() -> int {
        if (!b) { set_error("mrgfe_batch_align_best: NULL argument"); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(b->ctx);  // held over both stages: nothing else reaches the context while the selection is pending
        MRGFE_TRY(check_best_args(b, fitness_max_range, score_cap, group, n_groups, results, best, best_score));
        const int    P = b->book.n_pairs();
        const size_t N = static_cast<size_t>(std::max(P, 1));
        std::vector<double> lo(N), hi(N);
        MRGFE_TRY(batch_align_bounds(b, fitness_max_range, group, results, lo.data(), hi.data()));
        // the selection over the pairs that have a fitness job; every other pair (an empty cloud; grouped and not converged) is SKIPPED
        const std::vector<int>& job_pair = b->select.job_pair;
        const size_t J = job_pair.size();
        std::vector<int32_t> jgroup(J), jconv(J), jstate(J), state(N, kFitSkipped);
        std::vector<double>  jlo(J), jhi(J);
        for (size_t j = 0; j < J; ++j) { const int i = job_pair[j]; jgroup[j] = group[i]; jconv[j] = results[i].converged; jlo[j] = lo[i]; jhi[j] = hi[i]; }
        fit_select_prune(static_cast<int>(J), jlo.data(), jhi.data(), jconv.data(), jgroup.data(), n_groups, score_cap, jstate.data());
        for (size_t j = 0; j < J; ++j) state[job_pair[j]] = jstate[j];
        MRGFE_TRY(batch_align_finish(b, state.data(), results));
        std::vector<double>  fit(N);
        std::vector<int32_t> conv(N);
        for (int i = 0; i < P; ++i) { fit[i] = results[i].fitness; conv[i] = results[i].converged; }
        fit_select_groups(P, fit.data(), conv.data(), group, n_groups, score_cap, best, best_score);
        if (fit_state) std::memcpy(fit_state, state.data(), sizeof(int32_t) * static_cast<size_t>(P));
        return MRGFE_OK;
    });
}

int mrgfe_batch_select_stats(const mrgfe_batch* b, double out[8])
{
    if (!b || !out) { set_error("mrgfe_batch_select_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    const FitSelectStats& s = b->select_stats;
    const double v[8] = {double(s.exact), double(s.pruned), double(s.above_cap), double(s.skipped), double(s.to_sweep), double(s.to_far), s.ms_bound, s.ms_contend};
    std::memcpy(out, v, sizeof(v));
    return MRGFE_OK;
}

int mrgfe_dbg_batch_fit_bounds(const mrgfe_batch* b, double* lower, double* upper)
{
    if (!b || !lower || !upper) { set_error("mrgfe_dbg_batch_fit_bounds: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    if (b->fit_lo.size() != static_cast<size_t>(b->book.n_pairs())) { set_error("mrgfe_dbg_batch_fit_bounds: no mrgfe_batch_align_best on this pair list"); return MRGFE_ERR_STATE; }
    std::copy(b->fit_lo.begin(), b->fit_lo.end(), lower);
    std::copy(b->fit_hi.begin(), b->fit_hi.end(), upper);
    return MRGFE_OK;
}

int mrgfe_dbg_batch_ndt_rounds(const mrgfe_batch* b, int cap, uint32_t* n_pairs, uint32_t* n_items)
{
    if (!b || !b->ndt || cap < 0) { set_error("mrgfe_dbg_batch_ndt_rounds: needs an NDT batch"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    return b->ndt->round_info(cap, n_pairs, n_items);
}

// mrgfe_batch_timing, and the caller's clouds, at the end of an align that started at `t_start` and ended with status `st`
static int batch_align_ended(mrgfe_batch* b, std::chrono::steady_clock::time_point t_start, int st)
{
    if (st == MRGFE_OK) {
        b->last_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count();
        b->last_pairs = b->book.n_pairs();
        b->total_us += b->last_us;
        b->total_pairs += b->last_pairs;
    }
    // zero-copy uploads (mrgfe_ctx_set_zero_copy_uploads): the caller's page-locked clouds are its own again when this call returns — also when it fails
    // with their DMA still queued.  The error text of the failure is kept.
    if (st != MRGFE_OK && b->ctx->dma_from_caller) {
        const std::string msg = mrgfe_last_error();
        drain_caller_dma(b->ctx);
        set_error("%s", msg.c_str());
    } else {
        b->ctx->dma_from_caller = false;  // a successful align has waited for its stream
    }
    return st;
}

static int batch_align_timed(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results)
{
    MRGFE_LOCK(b->ctx);
    const auto t_start = b->t_queue_set ? b->t_queue : std::chrono::steady_clock::now();
    int st;
    {
        TraceRange tr("mrgfe_batch_align");
        st = batch_align_impl(b, fitness_max_range, results);
    }
    b->t_queue_set = false;
    return batch_align_ended(b, t_start, st);
}

}  // extern "C"

// ---- mrgfe_batch_align_best in two stages (api_internal.h): the callers are mrgfe_batch_align_best, which decides between them over this batch's
// pairs, and a node member (node.cpp), whose node decides over the pair lists of all its members
int batch_align_bounds(mrgfe_batch* b, double max_range, const int32_t* group, mrgfe_pair_result* results, double* lo, double* hi)
{
    MRGFE_LOCK(b->ctx);
    static const int32_t no_group = -1;
    if (!group) group = &no_group;  // (an empty pair list: nothing reads it, but "not null" is what asks for the selection)
    b->select.run.drop();
    b->select.t_start =b->t_queue_set ? b->t_queue : std::chrono::steady_clock::now();
    b->t_queue_set = false;
    int st;
    {
        TraceRange tr("mrgfe_batch_align_best: align and bounds");
        st = batch_align_impl(b, max_range, results, group);
    }
    if (st != MRGFE_OK) {
        b->select.run.drop();
        return batch_align_ended(b, b->select.t_start, st);
    }
    std::copy(b->fit_lo.begin(), b->fit_lo.end(), lo);
    std::copy(b->fit_hi.begin(), b->fit_hi.end(), hi);
    return MRGFE_OK;
}

int batch_align_finish(mrgfe_batch* b, const int32_t* state, mrgfe_pair_result* results)
{
    MRGFE_LOCK(b->ctx);
    if (!b->select.run.pending()) { set_error("batch_align_finish: no selection is pending on this batch"); return MRGFE_ERR_STATE; }
    TraceRange tr("mrgfe_batch_align_best: contenders");
    const std::vector<int>& job_pair = b->select.job_pair;
    const size_t J = job_pair.size();
    std::vector<int32_t> jstate(J);
    std::vector<double>  fit(J);
    for (size_t j = 0; j < J; ++j) jstate[j] = state[job_pair[j]];
    int st = b->ctx->bind();
    if (st == MRGFE_OK) st = b->select.run.finish(jstate.data(), fit.data(), &b->select_stats);
    b->select.run.drop();
    if (st == MRGFE_OK) {
        for (size_t j = 0; j < J; ++j) results[job_pair[j]].fitness = fit[j];
        // the counts are per PAIR; a SKIPPED pair has fitness DBL_MAX (what the full path gives a pair with an empty cloud; so has every pair without a job)
        FitSelectStats& ss = b->select_stats;
        ss.exact = ss.pruned = ss.above_cap = ss.skipped = 0;
        for (int i = 0; i < b->book.n_pairs(); ++i) {
            switch (state[i]) {
                case kFitExact: ++ss.exact; break;
                case kFitPruned: ++ss.pruned; break;
                case kFitAboveCap: ++ss.above_cap; break;
                default: ++ss.skipped; results[i].fitness = DBL_MAX;
            }
        }
    }
    return batch_align_ended(b, b->select.t_start, st);
}

// (api_internal.h) a node member's replica of a store keyframe as a source: mrgfe_batch_add_pair_from_store without the lookup
int batch_add_pair_device_keyed(mrgfe_batch* b, int target, uint64_t key, const void* d_xyzi, size_t n, const float guess[16])
{
    static const char* fn = "batch_add_pair_device_keyed";
    return abi_guard(fn, [&]() -> int {
        MRGFE_TRY(check_count(n, fn));
        if (!b || !guess || key == 0) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        MRGFE_LOCK(b->ctx);
        return add_pair_device_keyed(b, fn, target, key, d_xyzi, n, guess);
    });
}

int batch_align_abandon(mrgfe_batch* b)
{
    MRGFE_LOCK(b->ctx);
    b->select.run.drop();
    MRGFE_TRY(b->ctx->bind());
    MRGFE_HIP_CHECK(hipStreamSynchronize(b->ctx->stream));
    if (b->ctx->side) MRGFE_HIP_CHECK(hipStreamSynchronize(b->ctx->side));
    b->ctx->dma_from_caller = false;  // whatever was queued has run
    return MRGFE_OK;
}

extern "C" {

// GICP_HIP: the candidates of a target share its covariances and correspondence grid, and all LM loops advance together (GicpBatch: one
// launch per kernel and round for the pairs still running); ICP_HIP: lock-step ICP rounds, no covariances; PCL_GICP_HIP / PCL_GICP_OMP_HIP: PCL's
// covariances, the BFGS loops of the pairs in lock step, a round per functor evaluation.  The records follow in batch_records.
static int gicp_align_batch(mrgfe_batch* b)
{
    const PairBook& book = b->book;
    const int P = book.n_pairs();
    MRGFE_TRY(b->ctx->bind());
    if (b->gicp.size() < static_cast<size_t>(book.n_targets())) b->gicp.resize(book.n_targets());
    if (!b->gicp_batch) b->gicp_batch = std::make_unique<GicpBatch>(b->ctx);
    b->gicp_pairs.resize(P);  // (pairs beyond P free their buffers)
    for (int i = 0; i < P; ++i) {
        const PairBook::Target& t = book.target(book.pair(i).target);
        std::unique_ptr<GicpEngine>& g = b->gicp[book.pair(i).target];
        if (!g) {
            g = std::make_unique<GicpEngine>(b->ctx, gicp_params_from(b->params));
            MRGFE_TRY(g->set_target(t.d_pts, t.n));
        }
        GicpBatchPair& bp = b->gicp_pairs[i];
        bp.ext_cov = nullptr;
        bp.ext_cov_k = nullptr;
        if (static_cast<size_t>(i) < b->pair_key.size() && b->pair_key[i]) {
            mrgfe_batch::Keyframe& kf = b->store.find(b->pair_key[i])->data;  // (in use since the pair was added: it is there, and stays where it is)
            bp.ext_cov = &kf.cov;
            bp.ext_cov_k = &kf.cov_k;
        }
    }
    if (b->params.method == MRGFE_ICP_HIP) return b->gicp_batch->align_all_icp(b->gicp, book, b->gicp_pairs);
    if (is_pcl_gicp(b->params.method)) return b->gicp_batch->align_all_pcl(b->gicp, book, b->gicp_pairs);
    return b->gicp_batch->align_all(b->gicp, book, b->gicp_pairs);
}

// The fitness work of an NDT batch that overlaps its alignment rounds.
// Grid builders: getFitnessScore needs an exact-NN grid per distinct target, and those depend on the target clouds only: they are built on
// helper contexts by extra host threads WHILE the alignment rounds run (their small launches fill the tails of the derivative kernels), instead
// of one after the other behind the alignment (64 targets: ~10 ms of a 65 ms step).  One grid is a dozen small launches and half a dozen host
// waits (bounding box, the adaptive cell size, the scan table): 64 of them in a row took 30 ms of wall time for 4 ms of kernels and outlasted
// the 17 ms of alignment they were meant to hide behind.  So the targets are dealt to builder threads, each with its own context.
// Early pass: the rounds of a batch end in a long tail — a few stragglers line-searching while most alignments have finished and the chip idles
// between their small launches — and getFitnessScore of a finished pair needs nothing but its final transformation.  A second host thread asks
// the aligning thread for a snapshot (NdtSnapshotPort) and runs the passes of the finished pairs with a complete grid on a helper context beside
// the remaining rounds.  A pair's score does not depend on the launch it is computed in (nn_fit_sum_kernel's fixed slices), so the records are
// the same.
// The destructor joins every thread this object started: no return path can destroy a joinable std::thread, whose destructor would end the
// process (the SLAM node) instead of reporting the error.
struct FitOverlap {
    mrgfe_batch*       b;
    mrgfe_pair_result* results;
    double             max_range;
    bool               early_on = false;
    std::vector<char>  built;       // per target: its fitness grid is built in this call
    std::vector<char>  early_done;  // per pair: scored by the early pass
    std::vector<int>   todo;        // the targets the builders make, in chunks
    size_t             set_base = 0, sets_taken = 0;  // ... into b->fit_sets[set_base .. set_base + sets_taken)
    std::unique_ptr<std::atomic<char>[]> grid_ready;  // per target: its fitness grid is complete (set by the builder that made it)
    std::vector<std::thread> threads;
    std::mutex         mu;
    int                status = MRGFE_OK;  // the first error a thread reported, and its text
    std::string        error;

    ~FitOverlap() { join(); }
    void fail(int st, const std::string& why)
    {
        std::lock_guard<std::mutex> g(mu);
        if (status == MRGFE_OK) { status = st; error = why; }
    }
    void join()
    {
        if (b->port) b->port->finished.store(1, std::memory_order_release);  // (align_all says so too when it returns): no snapshot comes
        for (std::thread& t : threads) t.join();
        threads.clear();
    }
    int start(bool select)
    {
        const PairBook& e = b->book;
        const int  P = e.n_pairs();
        const bool overlap = max_range >= 0 && P >= 2 && std::getenv("MRGFE_NO_FIT_OVERLAP") == nullptr;
        // Round 4 ran an early wave whenever a sixth of the pairs had finished: the chip is still full of derivative work then, and the waves
        // only added their fixed costs (config[3], 256 pairs: 27.8 ms without them, 28.7 ms with).  What IS idle is the tail: a few stragglers
        // line-searching through tens of small rounds (one pair: ~12 us of derivative work on a chip that holds twenty times that).  So ONE pass,
        // started when the pairs still running drop to an eighth of the batch (MRGFE_EARLY_FIT_ACTIVE_DIV), scores every finished pair beside the
        // stragglers' rounds; the stragglers are scored behind the last round as before.  The count comes from the round plans the device
        // already publishes (no extra kernel until the one snapshot that carries the final transformations).
        int early_min_pairs = 8;
        if (const char* env = std::getenv("MRGFE_EARLY_FIT_MIN_PAIRS")) early_min_pairs = std::max(2, std::atoi(env));
        int early_div = 8;
        if (const char* env = std::getenv("MRGFE_EARLY_FIT_ACTIVE_DIV")) early_div = std::max(1, std::atoi(env));
        // (not in mrgfe_batch_align_best: the pass would score pairs exactly before their group's bounds are known)
        early_on = overlap && !select && P >= early_min_pairs && std::getenv("MRGFE_NO_EARLY_FIT") == nullptr;
        if (!b->port) b->port.reset(new NdtSnapshotPort());
        NdtSnapshotPort& port = *b->port;  // (its pinned buffer is kept between calls)
        if (early_on) MRGFE_TRY(port.buf.ensure(sizeof(NdtSnapshotHead) + sizeof(NdtSnapshotRec) * size_t(P)));
        if (overlap) {
            const int T = e.n_targets();
            built.resize(T, 0);
            if (b->fit_grids.size() < static_cast<size_t>(T)) b->fit_grids.resize(T);
            grid_ready.reset(new std::atomic<char>[std::max(1, T)]);
            // (a target whose grid an earlier align of these targets built — mrgfe_batch_clear_pairs — is ready as it stands)
            for (int t = 0; t < T; ++t) {
                const char valid = static_cast<size_t>(t) < b->fit_valid.size() ? b->fit_valid[t] : 0;
                built[t] = valid;
                grid_ready[t].store(valid, std::memory_order_relaxed);
            }
            for (int i = 0; i < P; ++i) {
                const PairBook::Pair& p = e.pair(i);
                if (e.target(p.target).n == 0 || p.n == 0 || built[p.target]) continue;
                built[p.target] = 1;
                todo.push_back(p.target);
            }
            // Each thread builds its targets a chunk at a time, every step of the build one launch over the chunk (NnGridSet).  ONE builder for up
            // to eight chunks, two beyond: a chunk's build is a dozen launches over all its targets, and a second thread's launches only compete
            // with the first's and with the rounds for the queues (config[3], 64 targets = 4 chunks: 25.9 - 26.2 ms per step with two builders,
            // 25.0 - 25.2 with one; the chunk size makes no difference from 8 to 64 targets)
            size_t n_builders = 0, chunk = 16;
            if (const char* env = std::getenv("MRGFE_FIT_BUILDERS")) n_builders = static_cast<size_t>(std::max(1, std::atoi(env)));
            if (const char* env = std::getenv("MRGFE_FIT_CHUNK")) chunk = static_cast<size_t>(std::max(1, std::atoi(env)));
            const size_t n_chunks = (todo.size() + chunk - 1) / chunk;
            if (n_builders == 0) n_builders = n_chunks > 8 ? 2 : 1;
            n_builders = std::min(n_builders, n_chunks);
            set_base = b->fit_sets_used;
            sets_taken = n_chunks;
            while (b->fit_sets.size() < set_base + n_chunks) b->fit_sets.emplace_back(new NnGridSet());
            while (b->fit_ctxs.size() < n_builders) {
                mrgfe_ctx* fc = nullptr;
                if (ctx_create_like(b->ctx, &fc) != MRGFE_OK) return MRGFE_ERR_HIP;  // (same compute-unit mask as the batch's own context)
                CtxPtr owned(fc);
                b->fit_ctxs.push_back(std::move(owned));
            }
            // the early fitness pass runs on a context of its own whose streams have the device's LOWEST priority: the stragglers' small launches
            // on the batch's stream are dispatched ahead of the pass's workgroups as slots free up (at equal priority the tail's rounds took twice
            // as long beside the pass: what the overlap gained, the rounds lost)
            if (early_on && !b->early_ctx) {
                mrgfe_ctx* ec = nullptr;
                if (ctx_create_like(b->ctx, &ec, -1) != MRGFE_OK) return MRGFE_ERR_HIP;
                b->early_ctx.reset(ec);
            }
            // the target clouds reach the device by asynchronous copies (and gathers) on the batch's stream: the helper streams
            // must not read them before those have finished
            MRGFE_TRY(b->ctx->bind());
            if (!b->uploads_done) MRGFE_HIP_CHECK(hipEventCreateWithFlags(&b->uploads_done, hipEventDisableTiming));
            MRGFE_HIP_CHECK(hipEventRecord(b->uploads_done, b->ctx->stream));
            for (size_t w = 0; w < n_builders; ++w)
                threads.emplace_back([this, w, n_builders, n_chunks, chunk] {
                    const PairBook& e = b->book;
                    mrgfe_ctx* fc = b->fit_ctxs[w].get();
                    std::lock_guard<std::recursive_mutex> lock(fc->mu);
                    if (fc->bind() != MRGFE_OK) { fail(MRGFE_ERR_HIP, mrgfe_last_error()); return; }
                    if (hipStreamWaitEvent(fc->stream, b->uploads_done, 0) != hipSuccess) { fail(MRGFE_ERR_HIP, "helper stream could not wait for the uploads"); return; }
                    std::vector<const float4*> clouds;
                    std::vector<uint32_t>      sizes;
                    std::vector<NnGrid*>       views;
                    for (size_t c = w; c < n_chunks; c += n_builders) {
                        const size_t k0 = c * chunk, k1 = std::min(todo.size(), k0 + chunk);
                        clouds.clear(); sizes.clear(); views.clear();
                        for (size_t k = k0; k < k1; ++k) {
                            const PairBook::Target& T = e.target(todo[k]);
                            clouds.push_back(T.d_pts);
                            sizes.push_back(static_cast<uint32_t>(T.n));
                            views.push_back(&b->fit_grids[todo[k]]);
                        }
                        const int st = b->fit_sets[set_base + c]->build(fc, clouds.data(), sizes.data(), static_cast<int>(k1 - k0), 1.0f, NnGrid::kCrowding1nn, 1, views.data());  // returns with the grids complete (synchronised)
                        if (st != MRGFE_OK) { fail(st, mrgfe_last_error()); return; }
                        for (size_t k = k0; k < k1; ++k) grid_ready[todo[k]].store(1, std::memory_order_release);
                    }
                    if (hipStreamSynchronize(fc->stream) != hipSuccess) fail(MRGFE_ERR_HIP, "helper stream synchronisation failed");
                });
        }
        port.want.store(0);
        port.issued.store(0);
        port.finished.store(0);
        early_done.assign(P, 0);
        b->fit_total = FitStats();
        if (!early_on) return MRGFE_OK;
        port.head()->tag = 0;
        port.n_active.store(static_cast<uint32_t>(P), std::memory_order_release);
        threads.emplace_back([this, P, early_div] {
            const PairBook& e = b->book;
            NdtSnapshotPort& port = *b->port;
            mrgfe_ctx* fc = b->early_ctx.get();
            std::lock_guard<std::recursive_mutex> lock(fc->mu);
            if (fc->bind() != MRGFE_OK) { fail(MRGFE_ERR_HIP, mrgfe_last_error()); return; }
            const uint32_t threshold = static_cast<uint32_t>(std::max(1, P / early_div));
            // wait for the tail (or the end of the alignment)
            while (!port.finished.load(std::memory_order_acquire) && port.n_active.load(std::memory_order_acquire) > threshold) std::this_thread::sleep_for(std::chrono::microseconds(20));
            if (port.finished.load(std::memory_order_acquire)) return;
            port.want.store(1, std::memory_order_release);
            while (port.issued.load(std::memory_order_acquire) == 0 && !port.finished.load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::microseconds(5));
            const uint32_t tag = port.issued.load(std::memory_order_acquire);
            if (tag == 0) return;  // finished without a snapshot
            volatile NdtSnapshotHead* hd = port.head();
            while (__atomic_load_n(&hd->tag, __ATOMIC_ACQUIRE) != tag) {
                if (port.finished.load(std::memory_order_acquire) && __atomic_load_n(&hd->tag, __ATOMIC_ACQUIRE) != tag) return;  // align_all failed before the kernel ran
                std::this_thread::sleep_for(std::chrono::microseconds(5));
            }
            std::vector<NnFitnessJob> jobs;
            std::vector<int>          job_pair;
            const NdtSnapshotRec* recs = port.recs();
            for (int i = 0; i < P; ++i) {
                if (!recs[i].done) continue;
                const PairBook::Pair& p = e.pair(i);
                if (e.target(p.target).n == 0 || p.n == 0 || !grid_ready[p.target].load(std::memory_order_acquire)) continue;
                float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
                std::memcpy(T, recs[i].T12, sizeof(recs[i].T12));
                jobs.push_back(b->fit_grids[p.target].make_fitness_job(p.d_src, p.n, T));
                job_pair.push_back(i);
            }
            if (jobs.empty()) return;
            std::vector<double> fit(jobs.size(), 0.0);
            TraceRange tr("mrgfe early fitness pass");
            const int st = nn_fitness_batch(fc, jobs.data(), jobs.size(), max_range, fit.data());
            if (st != MRGFE_OK) { fail(st, mrgfe_last_error()); return; }
            b->fit_total.add(fc->fit_stats);
            for (size_t j = 0; j < jobs.size(); ++j) { results[job_pair[j]].fitness = fit[j]; early_done[job_pair[j]] = 1; }
        });
        return MRGFE_OK;
    }
};

// The one writer of a mrgfe_pair_result: `final_rm` row-major, `hessian` 36 doubles or nullptr (a method without one: zeros).  The fitness is
// DBL_MAX until the fitness passes, unless the early pass has scored the pair already (`keep_fitness`).
static void write_record(mrgfe_pair_result& r, int pair, const float final_rm[16], const double* hessian, double trans_probability, bool converged, int iterations,
                         int evaluations, bool keep_fitness)
{
    row2col(final_rm, r.T);
    if (hessian) std::memcpy(r.H, hessian, sizeof(r.H));
    else         std::memset(r.H, 0, sizeof(r.H));
    if (!keep_fitness) r.fitness = DBL_MAX;
    r.trans_probability = trans_probability;
    r.converged = converged ? 1 : 0;
    r.iterations = iterations;
    r.evaluations = evaluations;
    r.pair_id = pair;
}

// after the rounds of any method: the final transformations (b->final_rm) and the records; the pairs the early pass scored keep their fitness
static void batch_records(mrgfe_batch* b, const std::vector<char>& early_done, mrgfe_pair_result* results)
{
    const int P = b->book.n_pairs();
    b->final_rm.assign(size_t(P) * 16, 0.0f);
    for (int i = 0; i < P; ++i) {
        float*     F = &b->final_rm[size_t(i) * 16];
        const bool scored = static_cast<size_t>(i) < early_done.size() && early_done[i];
        if (b->ndt) {
            const NdtController& c = b->ndt->ctl(i);
            std::memcpy(F, c.final_transformation(), sizeof(float) * 16);
            write_record(results[i], i, F, c.hessian(), c.trans_probability(), c.converged(), c.iterations(), c.evaluations(), scored);
        } else if (b->params.method == MRGFE_ICP_HIP) {  // no Hessian
            const IcpController& c = b->gicp_pairs[i].icp;
            std::memcpy(F, c.final_transformation(), sizeof(float) * 16);
            write_record(results[i], i, F, nullptr, 0.0, c.converged(), c.iterations(), c.evaluations(), scored);
        } else if (is_pcl_gicp(b->params.method)) {  // the BFGS keeps no Hessian
            const PclGicpController& c = b->gicp_pairs[i].pcl;
            std::memcpy(F, c.final_transformation(), sizeof(float) * 16);
            write_record(results[i], i, F, nullptr, 0.0, c.converged(), c.iterations(), c.evaluations(), scored);
        } else {
            const GicpLmController& c = b->gicp_pairs[i].ctl;
            c.final_transformation(F);
            write_record(results[i], i, F, c.hessian(), 0.0, c.converged(), c.iterations(), c.evaluations(), scored);
        }
    }
}

// The bound stage of the selection on the jobs (FitSelectRun::bounds: every job's interval); the run stays pending in b->select for batch_align_finish.
// The pairs without a job keep the interval DBL_MAX / DBL_MAX.
static int select_bounds(mrgfe_batch* b, double max_range, const mrgfe_pair_result* results, const int32_t* group, const std::vector<NnFitnessJob>& jobs, std::vector<int>& job_pair)
{
    const size_t J = jobs.size();
    std::vector<int32_t> jgroup(J), jconv(J);
    std::vector<double>  lo(J), hi(J);
    for (size_t j = 0; j < J; ++j) { jgroup[j] = group[job_pair[j]]; jconv[j] = results[job_pair[j]].converged; }
    b->select_stats = FitSelectStats();
    MRGFE_TRY(b->select.run.bounds(b->ctx, jobs.data(), J, max_range, jgroup.data(), jconv.data(), lo.data(), hi.data()));
    for (size_t j = 0; j < J; ++j) {
        b->fit_lo[job_pair[j]] = lo[j];
        b->fit_hi[job_pair[j]] = hi[j];
    }
    b->select.job_pair.swap(job_pair);
    return MRGFE_OK;
}

// getFitnessScore of every pair the early pass did not score, in one launch: one exact-NN grid per distinct target (built here unless a builder
// thread made it, `built`); with `sel_group` the bound stage of the bounded selection, where grouped pairs that did not converge are SKIPPED (never
// the best, no grid)
static int batch_fitness(mrgfe_batch* b, double max_range, mrgfe_pair_result* results, const int32_t* sel_group, std::vector<char>& built, const std::vector<char>& early_skip)
{
    TraceRange tr("mrgfe fitness passes");
    const PairBook& e = b->book;
    const int P = e.n_pairs();
    std::vector<NnGrid>& grids = b->fit_grids;
    if (grids.size() < static_cast<size_t>(e.n_targets())) grids.resize(e.n_targets());
    if (built.size() < static_cast<size_t>(e.n_targets())) built.resize(e.n_targets(), 0);
    if (b->fit_valid.size() < static_cast<size_t>(e.n_targets())) b->fit_valid.resize(e.n_targets(), 0);
    for (int t = 0; t < e.n_targets(); ++t) built[t] = built[t] || b->fit_valid[t];
    if (sel_group) {
        b->fit_lo.assign(P, DBL_MAX);
        b->fit_hi.assign(P, DBL_MAX);
    }
    std::vector<NnFitnessJob> jobs;
    std::vector<int>          job_pair;
    for (int i = 0; i < P; ++i) {
        const PairBook::Pair& p = e.pair(i);
        const PairBook::Target& t = e.target(p.target);
        if (t.n == 0 || p.n == 0 || (static_cast<size_t>(i) < early_skip.size() && early_skip[i])) continue;
        if (sel_group && sel_group[i] >= 0 && !results[i].converged) continue;
        if (!built[p.target]) { built[p.target] = 1; MRGFE_TRY(grids[p.target].build(b->ctx, t.d_pts, t.n, 1.0f, NnGrid::kCrowding1nn, 1)); }
        b->fit_valid[p.target] = 1;
        jobs.push_back(grids[p.target].make_fitness_job(p.d_src, p.n, &b->final_rm[size_t(i) * 16]));
        job_pair.push_back(i);
    }
    if (sel_group) return select_bounds(b, max_range, results, sel_group, jobs, job_pair);
    if (jobs.empty()) return MRGFE_OK;
    std::vector<double> fit(jobs.size());
    MRGFE_TRY(nn_fitness_batch(b->ctx, jobs.data(), jobs.size(), max_range, fit.data()));
    b->fit_total.add(b->ctx->fit_stats);
    for (size_t j = 0; j < jobs.size(); ++j) results[job_pair[j]].fitness = fit[j];
    return MRGFE_OK;
}

static int batch_align_impl(mrgfe_batch* b, double fitness_max_range, mrgfe_pair_result* results, const int32_t* sel_group)
{
    MRGFE_LOCK(b->ctx);
    std::vector<char> fit_built;   // targets whose fitness grid is built in this call
    std::vector<char> early_skip;  // pairs whose fitness score was computed beside the alignment rounds
    if (!sel_group) { b->fit_lo.clear(); b->fit_hi.clear(); }  // mrgfe_dbg_batch_fit_bounds: intervals of an align_best only
    if (!b->ndt) {
        MRGFE_TRY(gicp_align_batch(b));
        batch_records(b, early_skip, results);
    } else {
        FitOverlap ov{b, results, fitness_max_range};
        MRGFE_TRY(ov.start(sel_group != nullptr));
        int align_status;
        {
            TraceRange tr("mrgfe rounds (set_target + align_all)");
            align_status = b->ndt->align_all(ov.early_on ? b->port.get() : nullptr);
        }
        ov.join();
        MRGFE_TRY(align_status);
        if (ov.status != MRGFE_OK) { set_error("%s", ov.error.c_str()); return ov.status; }
        batch_records(b, ov.early_done, results);
        // the builders' grids are complete: they outlive the pairs (mrgfe_batch_clear_pairs), in sets no later build writes into
        if (b->fit_valid.size() < static_cast<size_t>(b->book.n_targets())) b->fit_valid.resize(b->book.n_targets(), 0);
        for (int t : ov.todo) b->fit_valid[t] = 1;
        if (ov.sets_taken) b->fit_sets_used = ov.set_base + ov.sets_taken;
        fit_built.swap(ov.built);
        early_skip.swap(ov.early_done);
    }
    return fitness_max_range >= 0 ? batch_fitness(b, fitness_max_range, results, sel_group, fit_built, early_skip) : MRGFE_OK;
}

int mrgfe_batch_fitness_stats(const mrgfe_batch* b, double out[11])
{
    if (!b || !out) { set_error("mrgfe_batch_fitness_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    const FitStats& f = b->fit_total;
    const double v[11] = {f.ms_block, f.ms_sweep, f.ms_far, double(f.queries), double(f.queued), double(f.queued_far), double(f.words), double(f.tested), double(f.cells), double(f.points), double(f.calls)};
    std::memcpy(out, v, sizeof(v));
    return MRGFE_OK;
}

int mrgfe_batch_timing(const mrgfe_batch* b, double out[4])
{
    if (!b || !out) { set_error("mrgfe_batch_timing: NULL argument"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    out[0] = b->total_pairs > 0 ? b->total_us / double(b->total_pairs) : 0.0;  // average_time_per_candidate_us (apps/mrg_slam_component.cpp:1032-1037)
    out[1] = b->last_us;
    out[2] = double(b->last_pairs);
    out[3] = double(b->total_pairs);
    return MRGFE_OK;
}
int mrgfe_batch_timing_reset(mrgfe_batch* b)
{
    if (!b) { set_error("mrgfe_batch_timing_reset: NULL batch"); return MRGFE_ERR_INVALID; }
    MRGFE_LOCK(b->ctx);
    b->last_us = b->total_us = 0.0;
    b->last_pairs = b->total_pairs = 0;
    return MRGFE_OK;
}

int mrgfe_batch_kernel_stats(const mrgfe_batch* b, int mode, double* ms, int64_t* launches, double* bytes)
{
    if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
    if (ms) *ms = 0;
    if (launches) *launches = 0;
    if (bytes) *bytes = 0;
    if (b->ndt) b->ndt->kernel_stats(mode, ms, launches, bytes);
    return MRGFE_OK;
}

int mrgfe_batch_largest_launch(const mrgfe_batch* b, double out[4])
{
    if (!b || !out) { set_error("mrgfe_batch_largest_launch: NULL argument"); return MRGFE_ERR_INVALID; }
    out[0] = b->ndt ? b->ndt->largest_ms : 0.0;
    for (int m = 0; m < 3; ++m) out[1 + m] = b->ndt ? double(b->ndt->largest_pairs[m]) : 0.0;
    return MRGFE_OK;
}

int mrgfe_batch_pair_counts(const mrgfe_batch* b, int mode, double* points, double* neighbours)
{
    if (!b) { set_error("NULL batch"); return MRGFE_ERR_INVALID; }
    double p = 0, n = 0;
    for (int m = 0; m < 3; ++m)
        if (b->ndt && (mode < 0 || mode == m)) { p += b->ndt->mode_points[m]; n += b->ndt->mode_neighbours[m]; }
    if (points) *points = p;
    if (neighbours) *neighbours = n;
    return MRGFE_OK;
}

int mrgfe_batch_rounds(const mrgfe_batch* b)
{
    if (!b) return 0;
    if (b->params.method == MRGFE_ICP_HIP || is_pcl_gicp(b->params.method)) return b->gicp_batch ? b->gicp_batch->rounds() : 0;
    return b->ndt ? b->ndt->rounds() : 0;
}

}  // extern "C"
