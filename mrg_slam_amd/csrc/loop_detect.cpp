// csrc/loop_detect.cpp — mrgfe_loop: LoopDetector::detect (src/mrg_slam/loop_detector.cpp:15-303) in one call over a batch and a map store.  The
// decisions are the controller's (loop_ctl.h, no HIP); this file checks the arguments, runs the two stages — on the borrowed batch through its public
// calls (stage 2 after mrgfe_batch_clear_pairs, on the targets stage 1 built), on a borrowed node through the same calls of mrgfe_node_*
// (mrgfe_loop_create_node), or through the aligner of mrgfe_dbg_loop_set_aligner — and hands the records to the replay.  Entry points follow the rules of api.cpp: codes and a thread-local message, no exception crosses.
#include <cfloat>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "loop_ctl.h"

using namespace mrgfe;

static_assert(sizeof(mrgfe_loop_params) == 72 && sizeof(mrgfe_loop_keyframe) == 432 && sizeof(mrgfe_loop_result) == 88, "record sizes of include/mrgfe.h");
static_assert(sizeof(LoopCtlKeyframe) == sizeof(mrgfe_loop_keyframe) && sizeof(LoopCtlLoop) == sizeof(mrgfe_loop_result), "loop_ctl.h mirrors the records field for field");

struct mrgfe_loop {
    std::mutex       mu;  // one detect at a time (the detector has no context of its own)
    mrgfe_batch*     batch = nullptr;
    mrgfe_node*      node = nullptr;   // mrgfe_loop_create_node: the stages run on it instead of the batch
    mrgfe_map_store* store = nullptr;
    mrgfe_loop_params params;
    LoopCtl          ctl;
    mrgfe_dbg_loop_aligner aligner = nullptr;
    void*            aligner_user = nullptr;
    bool             stage_reuse = true;
    int64_t          target_builds = 0;  // of the last successful call
};

static void ctl_params(const mrgfe_loop_params& p, LoopCtlParams* c)
{
    c->candidate_max_xy_distance = p.candidate_max_xy_distance;
    c->accum_distance_thresh_same_robot = p.accum_distance_thresh_same_robot;
    c->accum_distance_thresh_other_robot = p.accum_distance_thresh_other_robot;
    c->fitness_score_max_range = p.fitness_score_max_range;
    c->fitness_score_thresh = p.fitness_score_thresh;
    c->consistency_max_delta_trans = p.loop_closure_consistency_max_delta_trans;
    c->consistency_max_delta_angle = p.loop_closure_consistency_max_delta_angle;
    c->fitness_selection = p.fitness_selection;
    c->use_planar_registration_guess = p.use_planar_registration_guess;
    c->enable_consistency_check = p.enable_loop_closure_consistency_check;
}

static void to_ctl(const mrgfe_loop_keyframe* in, int n, std::vector<LoopCtlKeyframe>* out)
{
    out->resize(static_cast<size_t>(std::max(n, 0)));
    for (int i = 0; i < n; ++i) {
        LoopCtlKeyframe& k = (*out)[i];
        k.key = in[i].key;
        k.slam_id = in[i].slam_id;
        std::memcpy(k.estimate, in[i].estimate, sizeof(k.estimate));
        k.accum_distance = in[i].accum_distance;
        k.first_keyframe = in[i].first_keyframe;
        k.static_keyframe = in[i].static_keyframe;
        k.prev_key = in[i].prev_key;
        k.next_key = in[i].next_key;
        std::memcpy(k.prev_relpose, in[i].prev_relpose, sizeof(k.prev_relpose));
        std::memcpy(k.next_relpose, in[i].next_relpose, sizeof(k.next_relpose));
    }
}

namespace {
// one stage: the pairs of the controller against one target per new keyframe that has pairs.  `tid` (new keyframe -> target index) is made by stage 1
// and read by stage 2 when the targets are reused.
struct Stage {
    mrgfe_loop* d;
    const LoopCtlKeyframe* news;
    std::vector<int> tid;          // per new keyframe: its target index in the batch, -1: none yet
    int64_t targets_queued = 0;

    int run(int stage, const std::vector<LoopCtlPair>& pairs, bool want_fitness, int n_groups, std::vector<mrgfe_pair_result>* results)
    {
        const int P = static_cast<int>(pairs.size());
        results->assign(static_cast<size_t>(std::max(P, 1)), mrgfe_pair_result());
        std::memset(static_cast<void*>(results->data()), 0, sizeof(mrgfe_pair_result) * results->size());
        for (mrgfe_pair_result& r : *results) r.fitness = DBL_MAX;
        if (d->aligner) return run_aligner(stage, pairs, want_fitness, results);
        const bool reuse = stage == 2 && d->stage_reuse;
        if (d->node) return run_node(reuse, pairs, want_fitness, n_groups, results);
        if (reuse) {
            MRGFE_TRY(mrgfe_batch_clear_pairs(d->batch));
        } else {
            MRGFE_TRY(mrgfe_batch_clear(d->batch));
            std::fill(tid.begin(), tid.end(), -1);
        }
        for (const LoopCtlPair& pr : pairs) {
            if (tid[pr.k] < 0) {  // registration_->setInputTarget(new_keyframe->cloud), :104
                const int t = mrgfe_batch_add_target_from_store(d->batch, d->store, news[pr.k].key);
                if (t < 0) return t;
                tid[pr.k] = t;
                ++targets_queued;
            }
            const int pi = mrgfe_batch_add_pair_from_store(d->batch, tid[pr.k], d->store, pr.source_key, pr.guess);
            if (pi < 0) return pi;
        }
        if (!want_fitness) return mrgfe_batch_align(d->batch, -1.0, results->data());
        if (d->params.fitness_selection == 0) return mrgfe_batch_align(d->batch, d->params.fitness_score_max_range, results->data());
        // groups = (new keyframe, candidate's SLAM instance): the gates drop whole instances, and within a group a pruned record holds a lower bound
        // strictly above an exact score of the same group, so the best over any union of groups is unchanged; a group whose best exceeds
        // fitness_score_thresh (the cap) yields no loop either way
        std::vector<int32_t> group(static_cast<size_t>(std::max(P, 1))), best(static_cast<size_t>(std::max(n_groups, 1)));
        std::vector<double>  best_score(best.size());
        for (int i = 0; i < P; ++i) group[i] = pairs[i].group;
        return mrgfe_batch_align_best(d->batch, d->params.fitness_score_max_range, d->params.fitness_score_thresh, group.data(), n_groups, results->data(), nullptr, best.data(),
                                      best_score.data());
    }

    // the same stage over the GPUs of a node: the same list, groups and cap, through the node's forms of the same calls
    int run_node(bool reuse, const std::vector<LoopCtlPair>& pairs, bool want_fitness, int n_groups, std::vector<mrgfe_pair_result>* results)
    {
        const int P = static_cast<int>(pairs.size());
        if (reuse) {
            MRGFE_TRY(mrgfe_node_clear_pairs(d->node));
        } else {
            MRGFE_TRY(mrgfe_node_clear(d->node));
            std::fill(tid.begin(), tid.end(), -1);
        }
        for (const LoopCtlPair& pr : pairs) {
            if (tid[pr.k] < 0) {
                const int t = mrgfe_node_add_target_from_store(d->node, d->store, news[pr.k].key);
                if (t < 0) return t;
                tid[pr.k] = t;
                ++targets_queued;
            }
            const int pi = mrgfe_node_add_pair_from_store(d->node, tid[pr.k], d->store, pr.source_key, pr.guess);
            if (pi < 0) return pi;
        }
        if (!want_fitness) return mrgfe_node_align(d->node, -1.0, results->data());
        if (d->params.fitness_selection == 0) return mrgfe_node_align(d->node, d->params.fitness_score_max_range, results->data());
        std::vector<int32_t> group(static_cast<size_t>(std::max(P, 1))), best(static_cast<size_t>(std::max(n_groups, 1)));
        std::vector<double>  best_score(best.size());
        for (int i = 0; i < P; ++i) group[i] = pairs[i].group;
        return mrgfe_node_align_best(d->node, d->params.fitness_score_max_range, d->params.fitness_score_thresh, group.data(), n_groups, results->data(), nullptr, best.data(),
                                     best_score.data());
    }

    int run_aligner(int stage, const std::vector<LoopCtlPair>& pairs, bool want_fitness, std::vector<mrgfe_pair_result>* results)
    {
        const int P = static_cast<int>(pairs.size());
        std::vector<uint64_t> target_keys, source_keys(static_cast<size_t>(P));
        std::vector<int32_t>  pair_target(static_cast<size_t>(P));
        std::vector<float>    guesses(static_cast<size_t>(P) * 16);
        std::vector<int>      t_of(tid.size(), -1);
        for (int i = 0; i < P; ++i) {
            const LoopCtlPair& pr = pairs[i];
            if (t_of[pr.k] < 0) { t_of[pr.k] = static_cast<int>(target_keys.size()); target_keys.push_back(news[pr.k].key); }
            pair_target[i] = t_of[pr.k];
            source_keys[i] = pr.source_key;
            std::memcpy(&guesses[size_t(i) * 16], pr.guess, sizeof(pr.guess));
        }
        if (stage == 1) targets_queued += static_cast<int64_t>(target_keys.size());
        const int st = d->aligner(d->aligner_user, stage, static_cast<int>(target_keys.size()), target_keys.data(), P, pair_target.data(), source_keys.data(), guesses.data(),
                                  want_fitness ? 1 : 0, results->data());
        if (st != MRGFE_OK) set_error("mrgfe_loop_detect: the aligner of stage %d returned %d", stage, st);
        return st;
    }
};
}  // namespace

extern "C" {

void mrgfe_loop_default_params(mrgfe_loop_params* out)
{
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    const LoopCtlParams c;
    out->candidate_max_xy_distance = c.candidate_max_xy_distance;
    out->accum_distance_thresh_same_robot = c.accum_distance_thresh_same_robot;
    out->accum_distance_thresh_other_robot = c.accum_distance_thresh_other_robot;
    out->fitness_score_max_range = c.fitness_score_max_range;
    out->fitness_score_thresh = c.fitness_score_thresh;
    out->loop_closure_consistency_max_delta_trans = c.consistency_max_delta_trans;
    out->loop_closure_consistency_max_delta_angle = c.consistency_max_delta_angle;
    out->fitness_selection = c.fitness_selection;
    out->use_planar_registration_guess = c.use_planar_registration_guess;
    out->enable_loop_closure_consistency_check = c.enable_consistency_check;
}
size_t mrgfe_loop_params_size(void) { return sizeof(mrgfe_loop_params); }
size_t mrgfe_loop_keyframe_size(void) { return sizeof(mrgfe_loop_keyframe); }
size_t mrgfe_loop_result_size(void) { return sizeof(mrgfe_loop_result); }

int mrgfe_loop_create(mrgfe_batch* batch, mrgfe_map_store* store, const mrgfe_loop_params* params, mrgfe_loop** out)
{
    return abi_guard("mrgfe_loop_create", [&]() -> int {
        if (!out) { set_error("mrgfe_loop_create: NULL argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        if (!params || (batch == nullptr) != (store == nullptr)) { set_error("mrgfe_loop_create: NULL argument (batch and store are both given, or both NULL for a detector that gets an aligner)"); return MRGFE_ERR_INVALID; }
        if (params->fitness_selection != 0 && params->fitness_selection != 1) { set_error("mrgfe_loop_create: fitness_selection must be 0 (full) or 1 (bounded), not %d", params->fitness_selection); return MRGFE_ERR_INVALID; }
        mrgfe_loop* d = new (std::nothrow) mrgfe_loop();
        if (!d) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        d->batch = batch;
        d->store = store;
        d->params = *params;
        ctl_params(*params, &d->ctl.p);
        *out = d;
        return MRGFE_OK;
    });
}
int mrgfe_loop_create_node(mrgfe_node* node, mrgfe_map_store* store, const mrgfe_loop_params* params, mrgfe_loop** out)
{
    return abi_guard("mrgfe_loop_create_node", [&]() -> int {
        if (!out) { set_error("mrgfe_loop_create_node: NULL argument"); return MRGFE_ERR_INVALID; }
        *out = nullptr;
        if (!params || !node || !store) { set_error("mrgfe_loop_create_node: NULL argument"); return MRGFE_ERR_INVALID; }
        if (params->fitness_selection != 0 && params->fitness_selection != 1) { set_error("mrgfe_loop_create_node: fitness_selection must be 0 (full) or 1 (bounded), not %d", params->fitness_selection); return MRGFE_ERR_INVALID; }
        mrgfe_loop* d = new (std::nothrow) mrgfe_loop();
        if (!d) { set_error("out of host memory"); return MRGFE_ERR_INVALID; }
        d->node = node;
        d->store = store;
        d->params = *params;
        ctl_params(*params, &d->ctl.p);
        *out = d;
        return MRGFE_OK;
    });
}
void mrgfe_loop_destroy(mrgfe_loop* det) { delete det; }
int mrgfe_loop_reset(mrgfe_loop* det)
{
    if (!det) { set_error("mrgfe_loop_reset: NULL detector"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(det->mu);
    det->ctl.reset();
    det->ctl.superset_pairs = det->ctl.sequential_pairs = det->ctl.consistency_pairs = det->ctl.new_keyframes = 0;
    det->target_builds = 0;
    return MRGFE_OK;
}

int mrgfe_loop_detect(mrgfe_loop* det, int n_keyframes, const mrgfe_loop_keyframe* keyframes, int n_new, const mrgfe_loop_keyframe* new_keyframes, int n_edges,
                      const uint64_t* edge_keys, mrgfe_loop_result* loops_out, int capacity, int* n_loops)
{
    static const char* fn = "mrgfe_loop_detect";
    return abi_guard(fn, [&]() -> int {
        if (!det || !n_loops || capacity < 0 || (capacity > 0 && !loops_out)) { set_error("%s: NULL argument", fn); return MRGFE_ERR_INVALID; }
        *n_loops = 0;
        std::lock_guard<std::mutex> lk(det->mu);
        const auto t_start = std::chrono::steady_clock::now();
        LoopCtl& ctl = det->ctl;
        if (n_keyframes < 0 || n_new < 0 || n_edges < 0 || (n_keyframes && !keyframes) || (n_new && !new_keyframes) || (n_edges && !edge_keys)) {
            set_error("%s: a negative count or a NULL list", fn);
            return MRGFE_ERR_INVALID;
        }
        std::vector<LoopCtlKeyframe> kfs, news;
        to_ctl(keyframes, n_keyframes, &kfs);
        to_ctl(new_keyframes, n_new, &news);
        if (!ctl.plan(n_keyframes, kfs.data(), n_new, news.data(), n_edges, edge_keys)) { set_error("%s: %s", fn, ctl.error.c_str()); return MRGFE_ERR_INVALID; }
        const std::vector<LoopCtlPair>& pairs1 = ctl.stage1();
        if (pairs1.empty()) {  // no new keyframe, no keyframe or no candidate: nothing to align
            ctl.superset_pairs = ctl.sequential_pairs = ctl.consistency_pairs = 0;
            ctl.new_keyframes = n_new;
            det->target_builds = 0;
            return MRGFE_OK;
        }
        if (!det->aligner) {
            if ((!det->batch && !det->node) || !det->store) { set_error("%s: the detector has neither a batch and a store nor an aligner", fn); return MRGFE_ERR_STATE; }
            // every key the two stages can name, before anything is queued
            auto in_store = [&](uint64_t key) -> int {
                if (mrgfe_map_store_has(det->store, key, nullptr)) return MRGFE_OK;
                set_error("%s: keyframe %llu is not in the store", fn, static_cast<unsigned long long>(key));
                return MRGFE_ERR_INVALID;
            };
            for (const LoopCtlPair& pr : pairs1) { MRGFE_TRY(in_store(news[pr.k].key)); MRGFE_TRY(in_store(pr.source_key)); }
            for (uint64_t key : ctl.possible_consistency_keys()) MRGFE_TRY(in_store(key));
        }
        Stage stage{det, news.data(), std::vector<int>(static_cast<size_t>(n_new), -1)};
        std::vector<mrgfe_pair_result> res1, res2;
        MRGFE_TRY(stage.run(1, pairs1, true, ctl.n_groups(), &res1));
        std::vector<LoopCtlRecord> rec1(pairs1.size()), rec2;
        for (size_t i = 0; i < pairs1.size(); ++i) { std::memcpy(rec1[i].T, res1[i].T, sizeof(rec1[i].T)); rec1[i].converged = res1[i].converged; rec1[i].fitness = res1[i].fitness; }
        const std::vector<LoopCtlPair>& pairs2 = ctl.plan_consistency(rec1.data());
        if (!pairs2.empty()) {
            MRGFE_TRY(stage.run(2, pairs2, false, 0, &res2));
            rec2.resize(pairs2.size());
            for (size_t i = 0; i < pairs2.size(); ++i) { std::memcpy(rec2[i].T, res2[i].T, sizeof(rec2[i].T)); rec2[i].converged = res2[i].converged; rec2[i].fitness = res2[i].fitness; }
        }
        std::vector<LoopCtlLoop> found(static_cast<size_t>(std::max(capacity, 1)));
        const double elapsed_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count();
        const int n = ctl.replay(rec1.data(), rec2.data(), elapsed_us, found.data(), capacity);
        *n_loops = n;
        if (n > capacity) { set_error("%s: %d loops, room for %d", fn, n, capacity); return MRGFE_ERR_INVALID; }
        for (int i = 0; i < n; ++i) {
            loops_out[i].key1 = found[i].key1;
            loops_out[i].key2 = found[i].key2;
            std::memcpy(loops_out[i].relative_pose, found[i].relative_pose, sizeof(found[i].relative_pose));
            loops_out[i].score = found[i].score;
        }
        det->target_builds = stage.targets_queued;
        return MRGFE_OK;
    });
}

int mrgfe_loop_stats(const mrgfe_loop* det, int64_t out[5])
{
    if (!det || !out) { set_error("mrgfe_loop_stats: NULL argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_loop*>(det)->mu);
    out[0] = det->ctl.superset_pairs;
    out[1] = det->ctl.sequential_pairs;
    out[2] = det->ctl.consistency_pairs;
    out[3] = det->ctl.new_keyframes;
    out[4] = det->target_builds;
    return MRGFE_OK;
}

int mrgfe_loop_timing(const mrgfe_loop* det, int capacity, int32_t* candidates, int64_t* micros, int* n)
{
    if (!det || !n || capacity < 0 || (capacity > 0 && (!candidates || !micros))) { set_error("mrgfe_loop_timing: NULL argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_loop*>(det)->mu);
    const LoopCtl::State& s = det->ctl.state;
    *n = static_cast<int>(s.candidates_sizes.size());
    for (int i = 0; i < *n && i < capacity; ++i) { candidates[i] = s.candidates_sizes[i]; micros[i] = s.detection_times_us[i]; }
    return MRGFE_OK;
}

int mrgfe_loop_normalize_estimate(const double in[16], double out[16])
{
    if (!in || !out) { set_error("mrgfe_loop_normalize_estimate: NULL argument"); return MRGFE_ERR_INVALID; }
    loop_math::normalize_estimate(in, out);
    return MRGFE_OK;
}
int mrgfe_loop_guess(const double new_estimate_normalized[16], const double candidate_estimate[16], int planar, float guess[16])
{
    if (!new_estimate_normalized || !candidate_estimate || !guess) { set_error("mrgfe_loop_guess: NULL argument"); return MRGFE_ERR_INVALID; }
    loop_math::guess(new_estimate_normalized, candidate_estimate, planar, guess);
    return MRGFE_OK;
}

int mrgfe_dbg_loop_set_aligner(mrgfe_loop* det, mrgfe_dbg_loop_aligner fn, void* user)
{
    if (!det) { set_error("mrgfe_dbg_loop_set_aligner: NULL detector"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(det->mu);
    det->aligner = fn;
    det->aligner_user = user;
    return MRGFE_OK;
}
int mrgfe_dbg_loop_set_stage_reuse(mrgfe_loop* det, int on)
{
    if (!det) { set_error("mrgfe_dbg_loop_set_stage_reuse: NULL detector"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(det->mu);
    const int before = det->stage_reuse ? 1 : 0;
    det->stage_reuse = on != 0;
    return before;
}
int mrgfe_dbg_loop_manager(const mrgfe_loop* det, int capacity, uint64_t* out, int* n)
{
    if (!det || !n || capacity < 0 || (capacity > 0 && !out)) { set_error("mrgfe_dbg_loop_manager: NULL argument"); return MRGFE_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(const_cast<mrgfe_loop*>(det)->mu);
    int i = 0;
    for (const auto& kv : det->ctl.state.loops) {
        if (i < capacity) { out[4 * i] = kv.first.first; out[4 * i + 1] = kv.first.second; out[4 * i + 2] = kv.second.key1; out[4 * i + 3] = kv.second.key2; }
        ++i;
    }
    *n = i;
    return MRGFE_OK;
}

}  // extern "C"
