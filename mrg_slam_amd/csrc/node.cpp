// csrc/node.cpp — mrgfe_node_*: the multi-GPU form of the loop-closure candidate batch behind the C ABI.
//
// The reference's host is ONE C++ process per robot whose LoopDetector::matching walks the candidates of a new keyframe one
// after the other on one registration object (/root/reference/src/mrg_slam/loop_detector.cpp:104,126-145).  The alignments are
// independent, so a node object owns one MEMBER per GPU — a context, a batch (mrgfe_batch_*) and a host thread each — and
//   * cuts the declared pair list into contiguous blocks, one per member, sizes differing by at most one (the list is ordered by
//     new keyframe, so a block touches few distinct targets: the partitioning of mrg_slam_amd/loop_closure.py shard_indices);
//   * every member uploads / finds resident the clouds of ITS block, builds ITS targets and aligns ITS pairs on its GPU: no
//     data-path collective;
//   * the fixed-size 384-byte result records (pose, 6x6 Hessian, fitness, flags) are gathered into the caller's array — through
//     host memory, or with ONE ncclAllGather over the members' streams (RCCL over xGMI) when the members sit on distinct
//     devices and librccl can be loaded (dlopen: no link-time dependency);
//   * the caller replays the reference's sequential best-candidate rule on the gathered records (mrgfe_node_select_best), so the
//     answer does not depend on the number of GPUs.
// Members on the SAME device are allowed (several batches sharing one card): that is what a one-GPU box can test, bit for bit
// against a single batch, and RCCL — which refuses duplicate devices — is then not used.
// Never re-execs, never forks: threads only (a process that has initialised the GPU must not exec on this pool).
#include <dlfcn.h>

#include <atomic>
#include <cfloat>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "api_internal.h"
#include "fit_select.h"
#include "resident_cache.h"

using namespace mrgfe;

namespace {

// ---- RCCL through dlopen: only the five entry points the record gather needs (signatures of rccl.h) -------------------------------
typedef struct ncclComm* nccl_comm_t;
struct Rccl {
    void* lib = nullptr;
    int (*CommInitAll)(nccl_comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(nccl_comm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int /* ncclDataType_t */, nccl_comm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok() const { return lib && CommInitAll && CommDestroy && AllGather && GroupStart && GroupEnd; }
};
constexpr int kNcclChar = 0;  // ncclInt8 / ncclChar

Rccl& rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
        r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(r.lib, "ncclCommInitAll"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.lib, "ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.lib, "ncclGroupEnd"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    });
    return r;
}

// a cloud named by map-store key (mrgfe_node_add_*_from_store): where it lies, as the lookup at the add call found it (the store is append-only)
struct StoreRef {
    mrgfe_map_store* store = nullptr;  // null: a host-fed cloud
    const float4*    d = nullptr;
    int              device = -1;
};
struct TargetDecl {
    uint64_t     key;
    const float* xyzi;
    size_t       n, stride;
    StoreRef     from = {};
};
struct PairDecl {
    int          target;
    uint64_t     key;
    const float* xyzi;
    size_t       n, stride;
    float        guess[16];
    StoreRef     from = {};
};
// A member's resident clouds, one cache and one budget for both kinds: the caller's keyed targets and the replicas of map-store keyframes (as targets and as
// sources) — the same 64-bit key may name one of each.  An era is one member_fill; `held`: a target of the member's batch reads the cloud, which stays
// until the batch is cleared (mrgfe_node_clear_pairs keeps targets built).  n == 0 over a buffer: not known to be complete, filled again when next named.
enum CloudKind : uint8_t { kKeyedTarget = 0, kReplica = 1 };
using CloudKey = std::pair<CloudKind, uint64_t>;
struct ResidentCloud { DevBuf buf; size_t n = 0; size_t bytes() const { return buf.cap; } };
using Clouds = ResidentCache<CloudKey, ResidentCloud>;

// JOB_BOUNDS / JOB_FINISH: the two stages of mrgfe_node_align_best; JOB_ABANDON: give up a first stage that succeeded, because another member's failed
enum Job { JOB_NONE = 0, JOB_ALIGN = 1, JOB_QUIT = 2, JOB_BOUNDS = 3, JOB_FINISH = 4, JOB_ABANDON = 5 };
struct BatchDestroy { void operator()(mrgfe_batch* b) const { mrgfe_batch_destroy(b); } };

}  // namespace

struct mrgfe_node {
    struct Member {
        ~Member() { if (ctx) (void)hipSetDevice(device); }  // the members below free themselves on this device, in reverse order: the batch first, the context last
        int          index = 0, device = 0;
        CtxPtr       ctx;
        std::thread  th;                                        // (joined by mrgfe_node_destroy before the member goes)
        std::mutex   mu;
        std::condition_variable cv;
        Job          job = JOB_NONE;
        bool         done = true;
        int          status = MRGFE_OK;
        std::string  error;
        int          first = 0, count = 0;  // this member's block of the pair list
        std::vector<mrgfe_pair_result> local;
        Clouds       clouds;                                    // bounded (MRGFE_KEYFRAME_STORE_MB, a budget beside the batch store's): in the LoopDetector flow every keyframe is a target once
        // mrgfe_node_clear_pairs: the targets the member's batch holds, node target index -> index in the batch, good while batch_gen is the node's target_gen
        std::unordered_map<int, int> built;
        uint64_t     batch_gen = 0;                             // 0: the batch's targets are not to be reused (never filled, a failed call, mrgfe_node_forget)
        int64_t      store_stat[4] = {0, 0, 0, 0};              // mrgfe_node_store_stats, this member's part of the last align
        DevBuf       d_send, d_recv;                            // RCCL gather
        int          fail_next = 0;                             // test hook
        bool         staged = false;                            // mrgfe_node_align_best: this member's first stage succeeded and its selection is pending
        std::unique_ptr<mrgfe_batch, BatchDestroy> batch;
    };
    mrgfe_reg_params         params;
    std::vector<std::unique_ptr<Member>> members;
    std::vector<TargetDecl>  targets;
    std::vector<PairDecl>    pairs;
    uint64_t                 target_gen = 1;     // counts mrgfe_node_clear: the target indices mean the same clouds while it stands
    bool                     keep_targets = false;  // mrgfe_node_clear_pairs since the last mrgfe_node_clear: members keep what they built for these targets
    int                      store_copy = 0;     // mrgfe_dbg_node_set_store_copy
    double                   fitness_max_range = -1.0;
    std::vector<nccl_comm_t> comms;     // one per member when the RCCL gather is in use
    bool                     rccl_tried = false;
    int                      last_gather = 0;  // 0 host, 1 RCCL
    // mrgfe_node_align_best, per pair of the whole list: the caller's groups, what the members' first stages report (each member writes its own block),
    // and the states the calling thread decides between the stages
    const int32_t*           sel_group = nullptr;
    std::vector<double>      sel_lo, sel_hi;
    std::vector<int32_t>     sel_conv, sel_state;
    bool                     last_best = false;  // the last align was a successful align_best: sel_lo / sel_hi are its intervals
    double                   select_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::mutex               api_mu;    // one align at a time
};

namespace {

using Member = mrgfe_node::Member;

int member_fail(Member& m, int status)
{
    m.status = status;
    m.error = mrgfe_last_error();
    m.batch_gen = 0;  // whatever the batch holds now, the next call starts it afresh
    return status;
}

// The member's resident cloud under `key` with `n` points: found, or filled by `fill(dst)` — a host upload, a same-device copy or a peer copy on the member's
// stream — after room was made under the member's cap.  A keyed target grows in place; a replica is filled once, so it is allocated exactly
// (mrgfe_node_store_bytes counts 16 bytes per point) and counted in store_stat.  `have_source`: there is something to fill it from.
template <class Fill>
int member_cloud(Member& m, CloudKey key, size_t n, bool have_source, Fill fill, Clouds::Entry** out)
{
    const bool  replica = key.first == kReplica;
    const char* what = replica ? "keyframe" : "target key";
    const unsigned long long k = key.second;
    Clouds::Entry* e = m.clouds.find_or_insert(key);
    if (!e) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
    m.clouds.touch(*e);
    *out = e;
    ResidentCloud& c = e->data;
    if (c.n == n && c.buf.p) return MRGFE_OK;
    if (!have_source) { set_error("member %d: %s %llu is not resident and no cloud was given", m.index, what, k); return MRGFE_ERR_INVALID; }
    if (e->held) { set_error("member %d: %s %llu is held with %zu points under a built target and named with %zu", m.index, what, k, c.n, n); return MRGFE_ERR_INVALID; }
    const size_t bytes = std::max<size_t>(n, 1) * 16;
    MRGFE_LOCK(m.ctx);
    MRGFE_TRY(m.ctx->bind());
    c.n = 0;
    if (replica) c.buf.release();
    m.clouds.make_room(bytes);
    MRGFE_TRY(replica ? c.buf.ensure_exact(bytes) : c.buf.ensure(bytes));
    MRGFE_TRY(fill(c.buf.p));
    c.n = n;
    if (replica) { m.store_stat[1] += 1; m.store_stat[2] += static_cast<int64_t>(n * 16); }
    return MRGFE_OK;
}

// keyframe `key` of a map store on this member's device: the replica kept under the key, copied store device -> member device on the member's stream when it
// is not there (the runtime stages the copy where peer access is not enabled)
int member_replica(Member& m, uint64_t key, size_t n, const StoreRef& from, Clouds::Entry** out)
{
    return member_cloud(m, CloudKey{kReplica, key}, n, true, [&](void* dst) -> int {
        if (n && from.device == m.device) MRGFE_HIP_CHECK(hipMemcpyAsync(dst, from.d, n * 16, hipMemcpyDeviceToDevice, m.ctx->stream));
        else if (n)                       MRGFE_HIP_CHECK(hipMemcpyPeerAsync(dst, m.device, from.d, from.device, n * 16, m.ctx->stream));
        return MRGFE_OK;
    }, out);
}

// the member's block into its batch: targets in order of first use, pairs in list order (nothing for an empty block).  After mrgfe_node_clear_pairs the
// batch keeps the targets it holds (mrgfe_batch_clear_pairs) and only those the block needs and lacks are added.
int member_fill(mrgfe_node* node, Member& m)
{
    m.status = MRGFE_OK;
    m.error.clear();
    m.local.assign(static_cast<size_t>(m.count), mrgfe_pair_result{});
    std::fill(m.store_stat, m.store_stat + 4, int64_t(0));
#ifdef MRGFE_TESTING
    if (m.fail_next) {
        m.fail_next = 0;
        set_error("member %d: failure injected by mrgfe_dbg_node_fail_member", m.index);
        return member_fail(m, MRGFE_ERR_STATE);
    }
#endif
    if (m.count == 0) return MRGFE_OK;
    m.clouds.next_era();
    const bool reuse = node->keep_targets && m.batch_gen == node->target_gen;
    m.batch_gen = 0;  // until the block is in
    int st = reuse ? mrgfe_batch_clear_pairs(m.batch.get()) : mrgfe_batch_clear(m.batch.get());
    if (st != MRGFE_OK) return member_fail(m, st);
    if (!reuse) {
        m.built.clear();
        m.clouds.clear_held();
    }
    std::unordered_map<int, int> local_target;
    for (int i = m.first; i < m.first + m.count; ++i) {
        const PairDecl& p = node->pairs[static_cast<size_t>(i)];
        auto it = local_target.find(p.target);
        if (it == local_target.end()) {
            const TargetDecl& t = node->targets[static_cast<size_t>(p.target)];
            int ti;
            auto bt = m.built.find(p.target);
            if (bt != m.built.end()) {
                ti = bt->second;  // built by an earlier align on this target list
                ++m.store_stat[3];
            } else if (t.from.store && t.from.device == m.device && node->store_copy == 0) {
                ti = mrgfe_batch_add_target_from_store(m.batch.get(), t.from.store, t.key);
                ++m.store_stat[0];
            } else if (t.from.store || t.key) {
                // a replica of a store keyframe, or a keyed target: resident on this member's device, filled once, found again by the next batches that name it
                Clouds::Entry* rc = nullptr;
                st = t.from.store ? member_replica(m, t.key, t.n, t.from, &rc)
                                  : member_cloud(m, CloudKey{kKeyedTarget, t.key}, t.n, t.xyzi || !t.n, [&](void* dst) { return upload_cloud(m.ctx.get(), t.xyzi, t.n, t.stride, dst); }, &rc);
                if (st != MRGFE_OK) return member_fail(m, st);
                rc->held = true;
                ti = mrgfe_batch_add_target_device(m.batch.get(), rc->data.buf.p, rc->data.n);
            } else {
                ti = mrgfe_batch_add_target(m.batch.get(), t.xyzi, t.n, t.stride);
            }
            if (ti < 0) return member_fail(m, ti);
            m.built[p.target] = ti;
            it = local_target.emplace(p.target, ti).first;
        }
        int pi;
        if (p.from.store) {
            if (p.from.device == m.device && node->store_copy == 0) {
                pi = mrgfe_batch_add_pair_from_store(m.batch.get(), it->second, p.from.store, p.key, p.guess);
                ++m.store_stat[0];
            } else {
                // (the covariances of the GICP family are cached in the batch under the key, as the route above caches them)
                Clouds::Entry* rc = nullptr;
                if ((st = member_replica(m, p.key, p.n, p.from, &rc)) != MRGFE_OK) return member_fail(m, st);
                pi = batch_add_pair_device_keyed(m.batch.get(), it->second, p.key, rc->data.buf.p, rc->data.n, p.guess);
            }
        } else {
            pi = p.key ? mrgfe_batch_add_pair_keyed(m.batch.get(), it->second, p.key, p.xyzi, p.n, p.stride, p.guess)
                       : mrgfe_batch_add_pair(m.batch.get(), it->second, p.xyzi, p.n, p.stride, p.guess);
        }
        if (pi < 0) return member_fail(m, pi);
    }
    if (m.store_stat[1]) {  // the replicas are complete before anything reads them, and a copy that failed fails this member here
        MRGFE_LOCK(m.ctx);
        if ((st = m.ctx->bind()) != MRGFE_OK) return member_fail(m, st);
        const hipError_t e = hipStreamSynchronize(m.ctx->stream);
        if (e != hipSuccess) {
            set_error("member %d: copying keyframes from the map store: %s", m.index, hipGetErrorString(e));
            for (auto& kv : m.clouds) if (kv.first.first == kReplica && m.clouds.named(kv.second)) kv.second.data.n = 0;  // (not known to be complete; member_fail has the batch cleared before they are named again)
            return member_fail(m, MRGFE_ERR_HIP);
        }
    }
    m.batch_gen = node->target_gen;
    return MRGFE_OK;
}

// mrgfe_node_align: the block, then the batch's own align
int member_align(mrgfe_node* node, Member& m)
{
    int st = member_fill(node, m);
    if (st != MRGFE_OK || m.count == 0) return st;
    st = mrgfe_batch_align(m.batch.get(), node->fitness_max_range, m.local.data());
    if (st != MRGFE_OK) return member_fail(m, st);
    for (int k = 0; k < m.count; ++k) m.local[static_cast<size_t>(k)].pair_id = m.first + k;  // the GLOBAL pair index
    return MRGFE_OK;
}

// mrgfe_node_align_best, first stage: the block, the align and the interval of every pair of the block, written with `converged` into the node's arrays
// at the block's place.  The selection stays pending in the member's batch (batch_align_bounds): nobody else can reach its context, the node's api_mu is held.
int member_bounds(mrgfe_node* node, Member& m)
{
    m.staged = false;
    int st = member_fill(node, m);
    if (st != MRGFE_OK || m.count == 0) return st;
    const size_t f = static_cast<size_t>(m.first);
    st = batch_align_bounds(m.batch.get(), node->fitness_max_range, node->sel_group + f, m.local.data(), node->sel_lo.data() + f, node->sel_hi.data() + f);
    if (st != MRGFE_OK) return member_fail(m, st);
    for (int k = 0; k < m.count; ++k) node->sel_conv[f + static_cast<size_t>(k)] = m.local[static_cast<size_t>(k)].converged;
    m.staged = true;
    return MRGFE_OK;
}

// second stage: the exact passes for the contenders of the block, by the states the node decided over the whole list
int member_finish(mrgfe_node* node, Member& m)
{
    if (m.count == 0) return MRGFE_OK;
    m.staged = false;  // batch_align_finish leaves nothing pending, whether it succeeds or fails
    const int st = batch_align_finish(m.batch.get(), node->sel_state.data() + m.first, m.local.data());
    if (st != MRGFE_OK) return member_fail(m, st);
    for (int k = 0; k < m.count; ++k) m.local[static_cast<size_t>(k)].pair_id = m.first + k;  // the GLOBAL pair index
    return MRGFE_OK;
}

void member_main(mrgfe_node* node, Member* m)
{
    for (;;) {
        Job job;
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv.wait(lk, [&] { return m->job != JOB_NONE; });
            job = m->job;
        }
        if (job == JOB_QUIT) return;
        if (job == JOB_ABANDON) {
            // (its own failure changes nothing the caller could act on: the error reported is the one of the member that made the call fail)
            (void)abi_guard("mrgfe_node_align_best member", [&] { return batch_align_abandon(m->batch.get()); });
            m->staged = false;
        }
        const int st = job == JOB_ABANDON ? MRGFE_OK : abi_guard("mrgfe_node_align member", [&] {
            return job == JOB_BOUNDS ? member_bounds(node, *m) : job == JOB_FINISH ? member_finish(node, *m) : member_align(node, *m);
        });
        if (st != MRGFE_OK && m->status == MRGFE_OK) member_fail(*m, st);  // an exception: the member did not get to record it
        if (st != MRGFE_OK) {
            // the member's clouds go up by DMA out of the caller's page-locked buffers (zero-copy uploads are always on for members) and a failing
            // block may have queued copies it never waited for: mrgfe_node_align hands the buffers back only after they have drained
            MRGFE_LOCK(m->ctx);
            drain_caller_dma(m->ctx.get());
        }
        {
            std::lock_guard<std::mutex> lk(m->mu);
            m->job = JOB_NONE;
            m->done = true;
        }
        m->cv.notify_all();
    }
}

void post(Member* m, Job job)
{
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->job = job;
        m->done = false;
    }
    m->cv.notify_all();
}
void wait_done(Member* m)
{
    std::unique_lock<std::mutex> lk(m->mu);
    m->cv.wait(lk, [&] { return m->done; });
}

bool distinct_devices(const mrgfe_node* node)
{
    for (size_t a = 0; a < node->members.size(); ++a)
        for (size_t b = a + 1; b < node->members.size(); ++b)
            if (node->members[a]->device == node->members[b]->device) return false;
    return true;
}

// MRGFE_NODE_GATHER: "host" never uses RCCL, "rccl" uses it whenever the devices are distinct (also for ONE member: the code path a
// one-GPU box can exercise), unset: RCCL for two or more members on distinct devices
bool want_rccl(const mrgfe_node* node)
{
    const char* e = std::getenv("MRGFE_NODE_GATHER");
    if (e && std::strcmp(e, "host") == 0) return false;
    if (!distinct_devices(node)) return false;
    if (e && std::strcmp(e, "rccl") == 0) return true;
    return node->members.size() >= 2;
}

int rccl_setup(mrgfe_node* node)
{
    if (!node->comms.empty()) return MRGFE_OK;
    if (node->rccl_tried) return MRGFE_ERR_STATE;
    node->rccl_tried = true;
    Rccl& r = rccl();
    if (!r.ok()) { set_error("librccl could not be loaded"); return MRGFE_ERR_STATE; }
    std::vector<int> devs;
    for (auto& m : node->members) devs.push_back(m->device);
    node->comms.assign(devs.size(), nullptr);
    const int rc = r.CommInitAll(node->comms.data(), static_cast<int>(devs.size()), devs.data());
    if (rc != 0) {
        set_error("ncclCommInitAll failed: %s", r.GetErrorString ? r.GetErrorString(rc) : "?");
        node->comms.clear();
        return MRGFE_ERR_HIP;
    }
    return MRGFE_OK;
}

// one ncclAllGather of `per` records per member over the members' streams; member 0's receive buffer comes back to the host
int rccl_gather(mrgfe_node* node, int per, mrgfe_pair_result* results, int n_pairs)
{
    Rccl& r = rccl();
    const size_t G = node->members.size();
    const size_t rec = sizeof(mrgfe_pair_result), bytes = rec * static_cast<size_t>(per);
    std::vector<mrgfe_pair_result> pad(static_cast<size_t>(per));
    for (auto& m : node->members) {
        MRGFE_LOCK(m->ctx);
        MRGFE_TRY(m->ctx->bind());
        MRGFE_TRY(m->d_send.ensure(bytes));
        MRGFE_TRY(m->d_recv.ensure(bytes * G));
        for (int k = 0; k < per; ++k) {
            if (k < m->count) pad[static_cast<size_t>(k)] = m->local[static_cast<size_t>(k)];
            else { std::memset(&pad[static_cast<size_t>(k)], 0, rec); pad[static_cast<size_t>(k)].pair_id = -1; }
        }
        MRGFE_TRY(m->ctx->stage_h2d(m->d_send.p, pad.data(), bytes, m->ctx->stream));
    }
    int rc = r.GroupStart();
    for (size_t g = 0; g < G && rc == 0; ++g) {
        Member* m = node->members[g].get();
        (void)hipSetDevice(m->device);
        rc = r.AllGather(m->d_send.p, m->d_recv.p, bytes, kNcclChar, node->comms[g], m->ctx->stream);
    }
    const int rc_end = r.GroupEnd();
    if (rc == 0) rc = rc_end;
    if (rc != 0) { set_error("ncclAllGather failed: %s", r.GetErrorString ? r.GetErrorString(rc) : "?"); return MRGFE_ERR_HIP; }
    std::vector<mrgfe_pair_result> all(static_cast<size_t>(per) * G);
    {
        Member* m0 = node->members[0].get();
        MRGFE_LOCK(m0->ctx);
        MRGFE_TRY(m0->ctx->bind());
        MRGFE_HIP_CHECK(hipMemcpyAsync(all.data(), m0->d_recv.p, bytes * G, hipMemcpyDeviceToHost, m0->ctx->stream));
        MRGFE_HIP_CHECK(hipStreamSynchronize(m0->ctx->stream));
    }
    for (size_t g = 1; g < G; ++g) {  // every member's collective has to have finished before its buffers are reused
        Member* m = node->members[g].get();
        MRGFE_LOCK(m->ctx);
        MRGFE_TRY(m->ctx->bind());
        MRGFE_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
    }
    int seen = 0;
    for (const mrgfe_pair_result& x : all) {
        if (x.pair_id < 0) continue;
        if (x.pair_id >= n_pairs) { set_error("gathered record names pair %d of %d", x.pair_id, n_pairs); return MRGFE_ERR_STATE; }
        results[x.pair_id] = x;
        ++seen;
    }
    if (seen != n_pairs) { set_error("gathered %d records for %d pairs", seen, n_pairs); return MRGFE_ERR_STATE; }
    return MRGFE_OK;
}

// contiguous blocks, sizes differing by at most one, the first n mod G blocks the longer ones
void cut_blocks(mrgfe_node* node)
{
    const int n = static_cast<int>(node->pairs.size()), G = static_cast<int>(node->members.size());
    const int base = n / G, extra = n % G;
    for (int g = 0; g < G; ++g) {
        Member* m = node->members[static_cast<size_t>(g)].get();
        m->first = g * base + std::min(g, extra);
        m->count = base + (g < extra ? 1 : 0);
    }
}

// one job for every member, all waited for from the calling thread (a member that fails has finished too); the first member that failed names the error
int run_members(mrgfe_node* node, Job job, const char* fn, const char* what)
{
    {
        TraceRange tr(what);
        for (auto& m : node->members) post(m.get(), job);
        for (auto& m : node->members) wait_done(m.get());
    }
    for (auto& m : node->members)
        if (m->status != MRGFE_OK) {
            set_error("%s: member %d (device %d): %s", fn, m->index, m->device, m->error.c_str());
            return m->status;
        }
    return MRGFE_OK;
}

// the members' records into the caller's array in pair order: RCCL between distinct devices, host memory otherwise (want_rccl)
int gather_records(mrgfe_node* node, mrgfe_pair_result* results, int n)
{
    const int G = static_cast<int>(node->members.size());
    node->last_gather = 0;
    if (want_rccl(node) && rccl_setup(node) == MRGFE_OK) {
        const int per = (n + G - 1) / G;
        TraceRange tr("mrgfe_node_align record gather (RCCL)");
        const int st = rccl_gather(node, per, results, n);
        if (st == MRGFE_OK) { node->last_gather = 1; return MRGFE_OK; }
        if (const char* e = std::getenv("MRGFE_NODE_GATHER")) if (std::strcmp(e, "rccl") == 0) return st;  // asked for: do not hide the failure
    }
    for (auto& m : node->members)
        if (m->count) std::memcpy(results + m->first, m->local.data(), sizeof(mrgfe_pair_result) * static_cast<size_t>(m->count));
    return MRGFE_OK;
}

}  // namespace

extern "C" {

int mrgfe_node_create(int n_members, const int* device_ids, const mrgfe_reg_params* params, mrgfe_node** out)
{
    return abi_guard("mrgfe_node_create", [&]() -> int {
        if (!out || !params || n_members < 1 || n_members > 64 || !device_ids) { set_error("mrgfe_node_create: bad argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        std::unique_ptr<mrgfe_node> owned(new (std::nothrow) mrgfe_node());
        mrgfe_node* node = owned.get();
        if (!node) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        node->params = *params;
        int st = MRGFE_OK;
        for (int i = 0; i < n_members && st == MRGFE_OK; ++i) {
            std::unique_ptr<Member> fresh(new (std::nothrow) Member());
            if (!fresh) { set_error("out of host memory"); st = MRGFE_ERR_INVALID; break; }
            node->members.push_back(std::move(fresh));
            Member* m = node->members.back().get();
            m->index = i;
            m->device = device_ids[i];
            m->clouds.set_cap(Clouds::cap_from_env(size_t(16) << 30));
            mrgfe_ctx*   ctx = nullptr;
            mrgfe_batch* batch = nullptr;
            st = mrgfe_ctx_create(m->device, &ctx);
            m->ctx.reset(ctx);
            // (the node's clouds are declared by pointer and uploaded inside mrgfe_node_align, which returns after the members have finished: page-locked
            // ones can always go up by DMA from where they lie)
            if (st == MRGFE_OK) st = mrgfe_ctx_set_zero_copy_uploads(ctx, 1);
            if (st == MRGFE_OK) st = mrgfe_batch_create(ctx, params, &batch);
            m->batch.reset(batch);
        }
        // std::system_error (thread limit): an error code, never an exception across the C boundary
        if (st == MRGFE_OK && abi_guard("mrgfe_node_create: could not start a member thread", [&] {
                for (auto& m : node->members) m->th = std::thread(member_main, node, m.get());
                return MRGFE_OK;
            }) != MRGFE_OK)
            st = MRGFE_ERR_STATE;
        if (st != MRGFE_OK) {
            const std::string msg = mrgfe_last_error();
            mrgfe_node_destroy(owned.release());  // joins the members that did start
            set_error("%s", msg.c_str());
            return st;
        }
        *out = owned.release();
        return MRGFE_OK;
    });
}

void mrgfe_node_destroy(mrgfe_node* node)
{
    if (!node) return;
    for (auto& m : node->members) {
        if (m->th.joinable()) {
            wait_done(m.get());
            post(m.get(), JOB_QUIT);
            m->th.join();
        }
    }
    if (!node->comms.empty() && rccl().ok())
        for (nccl_comm_t c : node->comms) if (c) (void)rccl().CommDestroy(c);
    delete node;  // every member frees what it holds on its own device (Member)
}

int mrgfe_node_num_members(const mrgfe_node* node) { return node ? static_cast<int>(node->members.size()) : MRGFE_ERR_INVALID; }
int mrgfe_node_num_pairs(const mrgfe_node* node) { return node ? static_cast<int>(node->pairs.size()) : MRGFE_ERR_INVALID; }

int mrgfe_node_clear(mrgfe_node* node)
{
    return abi_guard("mrgfe_node_clear", [&]() -> int {
        if (!node) { set_error("mrgfe_node_clear: NULL node"); return MRGFE_ERR_INVALID; }
        std::lock_guard<std::mutex> lk(node->api_mu);
        node->targets.clear();
        node->pairs.clear();
        ++node->target_gen;
        node->keep_targets = false;
        return MRGFE_OK;
    });
}

int mrgfe_node_clear_pairs(mrgfe_node* node)
{
    return abi_guard("mrgfe_node_clear_pairs", [&]() -> int {
        if (!node) { set_error("mrgfe_node_clear_pairs: NULL node"); return MRGFE_ERR_INVALID; }
        std::lock_guard<std::mutex> lk(node->api_mu);
        node->pairs.clear();
        node->keep_targets = true;  // (a member whose batch was filled for another target list, or failed, starts afresh all the same: Member::batch_gen)
        return MRGFE_OK;
    });
}

int mrgfe_node_add_target_keyed(mrgfe_node* node, uint64_t cloud_key, const float* xyzi, size_t n, size_t stride_bytes)
{
    if (!node || (n && !xyzi && !cloud_key)) { set_error("mrgfe_node_add_target: NULL argument"); return MRGFE_ERR_INVALID; }
    if (n > 0x7fffffffu) { set_error("mrgfe_node_add_target: cloud too large"); return MRGFE_ERR_INVALID; }
    uint32_t s; uint32_t xo; int32_t io;
    if (decode_layout(stride_bytes, &s, &xo, &io) != MRGFE_OK) return MRGFE_ERR_INVALID;
    std::lock_guard<std::mutex> lk(node->api_mu);
    return abi_guard("mrgfe_node_add_target", [&] {
        node->targets.push_back(TargetDecl{cloud_key, xyzi, n, stride_bytes});
        return static_cast<int>(node->targets.size()) - 1;
    });
}
int mrgfe_node_add_target(mrgfe_node* node, const float* xyzi, size_t n, size_t stride_bytes) { return mrgfe_node_add_target_keyed(node, 0, xyzi, n, stride_bytes); }

int mrgfe_node_add_pair_keyed(mrgfe_node* node, int target_index, uint64_t cloud_key, const float* src_xyzi, size_t n, size_t stride_bytes, const float guess[16])
{
    if (!node || !guess || (n && !src_xyzi && !cloud_key)) { set_error("mrgfe_node_add_pair: NULL argument"); return MRGFE_ERR_INVALID; }
    if (n > 0x7fffffffu) { set_error("mrgfe_node_add_pair: cloud too large"); return MRGFE_ERR_INVALID; }
    uint32_t s; uint32_t xo; int32_t io;
    if (decode_layout(stride_bytes, &s, &xo, &io) != MRGFE_OK) return MRGFE_ERR_INVALID;
    std::lock_guard<std::mutex> lk(node->api_mu);
    if (target_index < 0 || target_index >= static_cast<int>(node->targets.size())) { set_error("mrgfe_node_add_pair: target index %d out of range", target_index); return MRGFE_ERR_INVALID; }
    PairDecl p;
    p.target = target_index; p.key = cloud_key; p.xyzi = src_xyzi; p.n = n; p.stride = stride_bytes;
    std::memcpy(p.guess, guess, sizeof(p.guess));
    return abi_guard("mrgfe_node_add_pair", [&] {
        node->pairs.push_back(p);
        return static_cast<int>(node->pairs.size()) - 1;
    });
}
int mrgfe_node_add_pair(mrgfe_node* node, int target_index, const float* src_xyzi, size_t n, size_t stride_bytes, const float guess[16])
{
    return mrgfe_node_add_pair_keyed(node, target_index, 0, src_xyzi, n, stride_bytes, guess);
}

int mrgfe_node_add_target_from_store(mrgfe_node* node, mrgfe_map_store* store, uint64_t key)
{
    static const char* fn = "mrgfe_node_add_target_from_store";
    return abi_guard(fn, [&]() -> int {
        if (!node || !store) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        StoreRef ref{store, nullptr, store->ctx->device};  // (the lookup takes the store's lock alone: it is released before the node's is taken)
        size_t n = 0;
        MRGFE_TRY(map_store_lookup(fn, store, key, &ref.d, &n));
        std::lock_guard<std::mutex> lk(node->api_mu);
        node->targets.push_back(TargetDecl{key, nullptr, n, 16, ref});
        return static_cast<int>(node->targets.size()) - 1;
    });
}

int mrgfe_node_add_pair_from_store(mrgfe_node* node, int target_index, mrgfe_map_store* store, uint64_t key, const float guess[16])
{
    static const char* fn = "mrgfe_node_add_pair_from_store";
    return abi_guard(fn, [&]() -> int {
        if (!node || !store || !guess) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        PairDecl p;
        p.target = target_index; p.key = key; p.xyzi = nullptr; p.stride = 16;
        std::memcpy(p.guess, guess, sizeof(p.guess));
        p.from.store = store; p.from.device = store->ctx->device;
        MRGFE_TRY(map_store_lookup(fn, store, key, &p.from.d, &p.n));
        std::lock_guard<std::mutex> lk(node->api_mu);
        if (target_index < 0 || target_index >= static_cast<int>(node->targets.size())) { set_error("%s: target index %d out of range", fn, target_index); return MRGFE_ERR_INVALID; }
        node->pairs.push_back(p);
        return static_cast<int>(node->pairs.size()) - 1;
    });
}

int mrgfe_node_store_stats(const mrgfe_node* node, int64_t out[4])
{
    if (!node || !out) { set_error("mrgfe_node_store_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_node*>(node)->api_mu);
    std::fill(out, out + 4, int64_t(0));
    for (auto& m : node->members)
        for (int k = 0; k < 4; ++k) out[k] += m->store_stat[k];
    return MRGFE_OK;
}

int mrgfe_dbg_node_set_store_copy(mrgfe_node* node, int mode)
{
    if (!node || (mode != 0 && mode != 1)) { set_error("mrgfe_dbg_node_set_store_copy: NULL node or a mode that is not 0 or 1"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(node->api_mu);
    node->store_copy = mode;
    return MRGFE_OK;
}

int mrgfe_node_align(mrgfe_node* node, double fitness_max_range, mrgfe_pair_result* results)
{
    return abi_guard("mrgfe_node_align", [&]() -> int {
        if (!node) { set_error("mrgfe_node_align: NULL node"); return MRGFE_ERR_INVALID; }
        std::lock_guard<std::mutex> lk(node->api_mu);
        const int n = static_cast<int>(node->pairs.size());
        if (n && !results) { set_error("mrgfe_node_align: NULL results"); return MRGFE_ERR_INVALID; }
        node->fitness_max_range = fitness_max_range;
        node->last_best = false;
        cut_blocks(node);
        // (after a failure the other members have finished their blocks and are idle again)
        MRGFE_TRY(run_members(node, JOB_ALIGN, "mrgfe_node_align", "mrgfe_node_align members"));
        if (n == 0) return MRGFE_OK;
        return gather_records(node, results, n);
    });
}

int mrgfe_node_align_best(mrgfe_node* node, double fitness_max_range, double score_cap, const int32_t* group, int n_groups, mrgfe_pair_result* results, int32_t* fit_state,
                          int32_t* best, double* best_score)
{
    static const char* fn = "mrgfe_node_align_best";
    return abi_guard(fn, [&]() -> int {
        if (!node || n_groups < 0 || (n_groups > 0 && (!best || !best_score))) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        std::lock_guard<std::mutex> lk(node->api_mu);
        const int    n = static_cast<int>(node->pairs.size());
        const size_t N = static_cast<size_t>(n);
        if (n && (!results || !group)) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        if (!(fitness_max_range >= 0) || std::isnan(score_cap)) { set_error("%s: fitness_max_range must be >= 0 and score_cap a number", fn); return MRGFE_ERR_INVALID; }
        for (int i = 0; i < n; ++i)
            if (group[i] < -1 || group[i] >= n_groups) { set_error("%s: group[%d] = %d is not -1 or in [0, %d)", fn, i, group[i], n_groups); return MRGFE_ERR_INVALID; }
        node->fitness_max_range = fitness_max_range;
        node->last_best = false;
        node->sel_group = group;
        node->sel_lo.assign(N, DBL_MAX);
        node->sel_hi.assign(N, DBL_MAX);
        node->sel_conv.assign(N, 0);
        node->sel_state.assign(N, kFitSkipped);
        std::fill(node->select_stats, node->select_stats + 8, 0.0);
        cut_blocks(node);
        if (n == 0) {  // one batch without pairs: every group is empty
            for (int g = 0; g < n_groups; ++g) { best[g] = -1; best_score[g] = DBL_MAX; }
            node->last_best = true;
            return MRGFE_OK;
        }
        // 1. every member: its block, the align, the intervals
        int st = run_members(node, JOB_BOUNDS, fn, "mrgfe_node_align_best members: align and bounds");
        if (st != MRGFE_OK) {
            // the members whose stage succeeded hold a pending selection and may still have work of this call queued: they give it up and wait for their
            // streams, so the caller's buffers are its own again.  (Posted from this thread like every job: a member that never got here cannot hold up another.)
            const std::string msg = mrgfe_last_error();
            for (auto& m : node->members) if (m->staged) post(m.get(), JOB_ABANDON);
            for (auto& m : node->members) wait_done(m.get());
            node->sel_group = nullptr;
            set_error("%s", msg.c_str());
            return st;
        }
        // 2. the selection over the WHOLE list.  A pair without a fitness job is SKIPPED as in one batch: an empty cloud (a grouped pair that did not
        // converge is SKIPPED by the rule itself); its interval DBL_MAX / DBL_MAX prunes nothing (no lower bound is above DBL_MAX)
        fit_select_prune(n, node->sel_lo.data(), node->sel_hi.data(), node->sel_conv.data(), group, n_groups, score_cap, node->sel_state.data());
        for (int i = 0; i < n; ++i) {
            const PairDecl& p = node->pairs[static_cast<size_t>(i)];
            if (p.n == 0 || node->targets[static_cast<size_t>(p.target)].n == 0) node->sel_state[static_cast<size_t>(i)] = kFitSkipped;
        }
        // 3. every member: the exact passes of its contenders.  A member that fails here has dropped its selection; the others have finished theirs.
        st = run_members(node, JOB_FINISH, fn, "mrgfe_node_align_best members: contenders");
        node->sel_group = nullptr;
        if (st != MRGFE_OK) return st;
        MRGFE_TRY(gather_records(node, results, n));
        // the rule on the gathered records; the states were decided here
        std::vector<double>  fit(N);
        std::vector<int32_t> conv(N);
        for (int i = 0; i < n; ++i) { fit[static_cast<size_t>(i)] = results[i].fitness; conv[static_cast<size_t>(i)] = results[i].converged; }
        fit_select_groups(n, fit.data(), conv.data(), group, n_groups, score_cap, best, best_score);
        if (fit_state) std::memcpy(fit_state, node->sel_state.data(), sizeof(int32_t) * N);
        for (auto& m : node->members) {
            if (!m->count) continue;
            double v[8];
            MRGFE_TRY(mrgfe_batch_select_stats(m->batch.get(), v));
            for (int k = 0; k < 6; ++k) node->select_stats[k] += v[k];
            for (int k = 6; k < 8; ++k) node->select_stats[k] = std::max(node->select_stats[k], v[k]);
        }
        node->last_best = true;
        return MRGFE_OK;
    });
}

int mrgfe_node_select_stats(const mrgfe_node* node, double out[8])
{
    if (!node || !out) { set_error("mrgfe_node_select_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_node*>(node)->api_mu);
    std::memcpy(out, node->select_stats, sizeof(node->select_stats));
    return MRGFE_OK;
}

int mrgfe_dbg_node_fit_bounds(const mrgfe_node* node, double* lower, double* upper)
{
    if (!node || !lower || !upper) { set_error("mrgfe_dbg_node_fit_bounds: NULL argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_node*>(node)->api_mu);
    if (!node->last_best || node->sel_lo.size() != node->pairs.size()) { set_error("mrgfe_dbg_node_fit_bounds: no mrgfe_node_align_best on this pair list"); return MRGFE_ERR_STATE; }
    std::copy(node->sel_lo.begin(), node->sel_lo.end(), lower);
    std::copy(node->sel_hi.begin(), node->sel_hi.end(), upper);
    return MRGFE_OK;
}

int mrgfe_dbg_node_ndt_rounds(const mrgfe_node* node, int member, int cap, uint32_t* n_pairs, uint32_t* n_items)
{
    if (!node || member < 0 || member >= static_cast<int>(node->members.size())) { set_error("mrgfe_dbg_node_ndt_rounds: bad argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_node*>(node)->api_mu);
    return mrgfe_dbg_batch_ndt_rounds(node->members[static_cast<size_t>(member)]->batch.get(), cap, n_pairs, n_items);
}

int mrgfe_node_shard(const mrgfe_node* node, int member, int* first_pair, int* n_pairs)
{
    if (!node || member < 0 || member >= static_cast<int>(node->members.size())) { set_error("mrgfe_node_shard: bad argument"); return MRGFE_ERR_INVALID; }
    if (first_pair) *first_pair = node->members[static_cast<size_t>(member)]->first;
    if (n_pairs) *n_pairs = node->members[static_cast<size_t>(member)]->count;
    return MRGFE_OK;
}

int mrgfe_node_last_gather(const mrgfe_node* node) { return node ? node->last_gather : MRGFE_ERR_INVALID; }

int mrgfe_node_forget(mrgfe_node* node, uint64_t cloud_key)
{
    return abi_guard("mrgfe_node_forget", [&]() -> int {
        if (!node) { set_error("mrgfe_node_forget: NULL node"); return MRGFE_ERR_INVALID; }
        std::lock_guard<std::mutex> lk(node->api_mu);
        for (auto& m : node->members) {
            {
                MRGFE_LOCK(m->ctx);
                (void)m->ctx->bind();
                if (cloud_key == 0) m->clouds.clear();
                for (CloudKind kind : {kKeyedTarget, kReplica}) m->clouds.erase(CloudKey{kind, cloud_key});
                m->clouds.clear_held();  // (the batch is cleared below)
                m->built.clear();
                m->batch_gen = 0;
            }
            MRGFE_TRY(mrgfe_batch_clear(m->batch.get()));  // the member's last block still references its clouds; the node's own list is re-declared per call anyway
            MRGFE_TRY(mrgfe_batch_forget(m->batch.get(), cloud_key));
        }
        return MRGFE_OK;
    });
}

size_t mrgfe_node_store_bytes(const mrgfe_node* node)
{
    if (!node) return 0;
    size_t total = 0;
    for (auto& m : node->members) {
        total += mrgfe_batch_store_bytes(m->batch.get()) + m->clouds.bytes();
    }
    return total;
}

int mrgfe_node_select_best(const mrgfe_pair_result* results, int n_groups, const int32_t* group_first, int32_t* best, double* best_score)
{
    if ((n_groups > 0 && (!results || !group_first)) || n_groups < 0) { set_error("mrgfe_node_select_best: bad argument"); return MRGFE_ERR_INVALID; }
    for (int g = 0; g < n_groups; ++g) {
        // loop_detector.cpp:126-145:  if( !hasConverged() || score > best_score ) continue;  best_score = score;  best_matched = candidate;
        double bs = DBL_MAX;
        int    b = -1;
        for (int i = group_first[g]; i < group_first[g + 1]; ++i) {
            const double score = results[i].fitness;
            if (!results[i].converged || score > bs) continue;
            bs = score;
            b = i - group_first[g];
        }
        if (best) best[g] = b;
        if (best_score) best_score[g] = bs;
    }
    return MRGFE_OK;
}

#ifdef MRGFE_TESTING
int mrgfe_dbg_node_fail_member(mrgfe_node* node, int member)
{
    if (!node || member < 0 || member >= static_cast<int>(node->members.size())) { set_error("mrgfe_dbg_node_fail_member: bad argument"); return MRGFE_ERR_INVALID; }
    node->members[static_cast<size_t>(member)]->fail_next = 1;
    return MRGFE_OK;
}
#endif

}  // extern "C"
