// csrc/loop_ctl.h — the state and the decisions of LoopDetector::detect (src/mrg_slam/loop_detector.cpp:15-303) as a controller the one-call detector
// (loop_detect.cpp) drives: plan() makes the candidate supersets (:41-76 without the LoopManager gates of :77-90) and the pair list of the first stage,
// plan_consistency() the pair list of the second (the previous / next keyframe of every best match any gate state can produce), replay() runs the
// reference's loop keyframe after keyframe on the records — the gates, the best-score rule (:137-144), the thresholds (:156-166), the consistency check
// (:190-303) and add_loop.  It is mrg_slam_amd/loop_detector.py::detect_batched step for step.  Header-only host code, no HIP:
// tests/sanitize/loop_ctl_san.cpp compiles it alone.
//
// Why the superset is enough: the gates only REMOVE candidates, and they drop all candidates of a SLAM instance or none (their conditions name the
// candidate's instance only).  So the candidate lists the replay can meet are the supersets minus any set of instances; the best match of each is known
// after the first stage, and the best of a union of instances is the best of one of them.
//
// Arithmetic.  Matrices are column-major 4x4, element (r, c) at [4 c + r], as in the C ABI.
//   * normalize_estimate (:183-188): Quaterniond(linear()).normalized().toRotationMatrix() in double, Eigen's conversions restated;
//   * guess (:124,129-133): Isometry3d::inverse() is the rigid inverse (R^T, -R^T t) in double, the product in double, the result cast to float;
//   * consistency deltas (:242-245, :285-291): Matrix4f products and the general float inverse (cofactors), the translation's float norm and
//     Quaternionf::angularDistance = 2 atan2(|vec|, |w|).  They have to give the mirror's decisions; their intermediate bits are not pinned.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace mrgfe {

struct LoopCtlParams {  // config/mrg_slam.yaml:169-179
    double  candidate_max_xy_distance = 15.0, accum_distance_thresh_same_robot = 15.0, accum_distance_thresh_other_robot = 5.0;
    double  fitness_score_max_range = HUGE_VAL, fitness_score_thresh = 1.25;
    double  consistency_max_delta_trans = 0.3, consistency_max_delta_angle = 0.0523599;
    int32_t fitness_selection = 0, use_planar_registration_guess = 0, enable_consistency_check = 1;
};

struct LoopCtlKeyframe {  // the slice of KeyFrame the detector reads
    uint64_t key = 0, slam_id = 0;
    double   estimate[16] = {0};
    double   accum_distance = 0;
    int32_t  first_keyframe = 0, static_keyframe = 0;
    uint64_t prev_key = 0, next_key = 0;  // 0: no edge
    double   prev_relpose[16] = {0}, next_relpose[16] = {0};
};

struct LoopCtlRecord {  // what the replay reads of a mrgfe_pair_result
    float   T[16];
    int32_t converged;
    double  fitness;
};

struct LoopCtlLoop {
    uint64_t key1, key2;
    float    relative_pose[16];
    double   score;
};

struct LoopCtlPair {  // one alignment: source keyframe against the cloud of new keyframe `k`
    int      k;
    uint64_t source_key;
    int32_t  group;  // stage 1: the (new keyframe, SLAM instance) group of the bounded selection
    float    guess[16];
};

namespace loop_math {
inline void quat_from_matrix_d(const double* m /* column-major 4x4 */, double q[4] /* w x y z */)
{
    auto R = [&](int r, int c) { return m[4 * c + r]; };
    double t = R(0, 0) + R(1, 1) + R(2, 2);
    q[0] = q[1] = q[2] = q[3] = 0.0;
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R(2, 1) - R(1, 2)) * t;
        q[2] = (R(0, 2) - R(2, 0)) * t;
        q[3] = (R(1, 0) - R(0, 1)) * t;
    } else {
        int i = 0;
        if (R(1, 1) > R(0, 0)) i = 1;
        if (R(2, 2) > R(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R(k, j) - R(j, k)) * t;
        q[1 + j] = (R(j, i) + R(i, j)) * t;
        q[1 + k] = (R(k, i) + R(i, k)) * t;
    }
}
inline void quat_from_matrix_f(const float* m, float q[4])
{
    auto R = [&](int r, int c) { return m[4 * c + r]; };
    float t = R(0, 0) + R(1, 1) + R(2, 2);
    q[0] = q[1] = q[2] = q[3] = 0.0f;
    if (t > 0) {
        t = std::sqrt(t + 1.0f);
        q[0] = 0.5f * t;
        t = 0.5f / t;
        q[1] = (R(2, 1) - R(1, 2)) * t;
        q[2] = (R(0, 2) - R(2, 0)) * t;
        q[3] = (R(1, 0) - R(0, 1)) * t;
    } else {
        int i = 0;
        if (R(1, 1) > R(0, 0)) i = 1;
        if (R(2, 2) > R(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0f);
        q[1 + i] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (R(k, j) - R(j, k)) * t;
        q[1 + j] = (R(j, i) + R(i, j)) * t;
        q[1 + k] = (R(k, i) + R(i, k)) * t;
    }
}
// :183-188
inline void normalize_estimate(const double in[16], double out[16])
{
    double q[4];
    quat_from_matrix_d(in, q);
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    double o[16];
    std::memcpy(o, in, sizeof(o));
    o[0] = 1 - (tyy + tzz); o[4] = txy - twz;       o[8] = txz + twy;
    o[1] = txy + twz;       o[5] = 1 - (txx + tzz); o[9] = tyz - twx;
    o[2] = txz - twy;       o[6] = tyz + twx;       o[10] = 1 - (txx + tyy);
    std::memcpy(out, o, sizeof(o));
}
// :129-133: (new_estimate.inverse() * normalize_estimate(candidate)).matrix().cast<float>(), z of the translation zeroed for the planar guess
inline void guess(const double new_normalized[16], const double candidate[16], int planar, float out[16])
{
    double c[16], inv[16] = {0};
    normalize_estimate(candidate, c);
    const double* a = new_normalized;
    for (int r = 0; r < 3; ++r) {
        for (int col = 0; col < 3; ++col) inv[4 * col + r] = a[4 * r + col];  // R^T
        inv[12 + r] = -(a[4 * r + 0] * a[12] + a[4 * r + 1] * a[13] + a[4 * r + 2] * a[14]);
    }
    inv[15] = 1.0;
    double g[16] = {0};
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 3; ++r) {
            double s = inv[r] * c[4 * col] + inv[4 + r] * c[4 * col + 1] + inv[8 + r] * c[4 * col + 2];
            if (col == 3) s += inv[12 + r];
            g[4 * col + r] = s;
        }
    g[15] = 1.0;
    for (int i = 0; i < 16; ++i) out[i] = static_cast<float>(g[i]);
    if (planar) out[14] = 0.0f;
}
inline void mul_f(const float a[16], const float b[16], float out[16])
{
    float t[16];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float s = a[r] * b[4 * c];
            for (int k = 1; k < 4; ++k) s += a[4 * k + r] * b[4 * c + k];
            t[4 * c + r] = s;
        }
    std::memcpy(out, t, sizeof(t));
}
// general 4x4 inverse by cofactors, in float (Matrix4f::inverse()); a singular matrix gives inf / NaN entries as the division does
inline void inverse_f(const float m[16], float out[16])
{
    float inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    const float s = 1.0f / det;
    for (int i = 0; i < 16; ++i) out[i] = inv[i] * s;
}
// Quaternionf(R).angularDistance(Quaternionf::Identity()) = 2 atan2(|vec|, |w|), in float
inline float angular_distance_to_identity(const float m[16])
{
    float q[4];
    quat_from_matrix_f(m, q);
    return 2.0f * std::atan2(std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), std::fabs(q[0]));
}
}  // namespace loop_math

class LoopCtl {
   public:
    LoopCtlParams p;

    // everything detect() keeps between calls: the LoopManager (loop_detector.hpp:39-115: the most recent loop per (new keyframe's instance,
    // candidate's instance)) and the reference's counters (:22-34)
    struct ManagerEntry { uint64_t key1, key2; double key1_accum_distance; };
    struct State {
        std::map<std::pair<uint64_t, uint64_t>, ManagerEntry> loops;
        std::vector<int32_t> candidates_sizes;
        std::vector<int64_t> detection_times_us;
    };
    State state;
    void  reset() { state = State(); }

    // the last call's counts (detect_batched's last_batched)
    int64_t superset_pairs = 0, sequential_pairs = 0, consistency_pairs = 0, new_keyframes = 0;

    std::string error;  // why the last plan() failed

    // ---- step 1: supersets and the first stage's pairs.  false: a bad argument (error says which); nothing was changed.
    bool plan(int n_keyframes, const LoopCtlKeyframe* keyframes, int n_new, const LoopCtlKeyframe* new_keyframes, int n_edges, const uint64_t* edge_keys)
    {
        error.clear();
        kfs_ = keyframes;
        news_ = new_keyframes;
        n_new_ = n_new;
        by_key_.clear();
        supersets_.clear();
        pairs1_.clear();
        pairs2_.clear();
        new_norm_.clear();
        if (n_keyframes < 0 || n_new < 0 || n_edges < 0 || (n_keyframes && !keyframes) || (n_new && !new_keyframes) || (n_edges && !edge_keys)) {
            error = "a negative count or a NULL list";
            return false;
        }
        for (int i = 0; i < n_keyframes; ++i) {
            if (keyframes[i].key == 0) { error = "keyframes[" + std::to_string(i) + "] has key 0"; return false; }
            by_key_[keyframes[i].key] = &keyframes[i];
        }
        for (int i = 0; i < n_new; ++i) {
            if (new_keyframes[i].key == 0) { error = "new_keyframes[" + std::to_string(i) + "] has key 0"; return false; }
            by_key_.emplace(new_keyframes[i].key, &new_keyframes[i]);
        }
        for (int i = 0; i < n_keyframes; ++i)
            for (uint64_t nb : {keyframes[i].prev_key, keyframes[i].next_key})
                if (nb != 0 && !by_key_.count(nb)) {
                    error = "keyframe " + std::to_string(keyframes[i].key) + " names the neighbour " + std::to_string(nb) + ", which is in neither list";
                    return false;
                }
        std::set<std::pair<uint64_t, uint64_t>> edges;
        for (int e = 0; e < n_edges; ++e) edges.insert(std::minmax(edge_keys[2 * e], edge_keys[2 * e + 1]));
        const double max_sq = p.candidate_max_xy_distance * p.candidate_max_xy_distance;
        supersets_.resize(n_new);
        new_norm_.resize(size_t(n_new) * 16);
        std::map<std::pair<int, uint64_t>, int32_t> gid;
        for (int k = 0; k < n_new; ++k) {
            const LoopCtlKeyframe& nk = new_keyframes[k];
            loop_math::normalize_estimate(nk.estimate, &new_norm_[size_t(k) * 16]);
            for (int i = 0; i < n_keyframes; ++i) {  // :41-76
                const LoopCtlKeyframe& c = keyframes[i];
                if (edges.count(std::minmax(nk.key, c.key))) continue;  // there is already an edge
                if (c.first_keyframe) continue;                         // first keyframes don't filter out points that hit other rovers
                const double dx = c.estimate[12] - nk.estimate[12], dy = c.estimate[13] - nk.estimate[13];
                if (dx * dx + dy * dy > max_sq) continue;
                if (nk.slam_id == c.slam_id && nk.accum_distance - c.accum_distance < p.accum_distance_thresh_same_robot) continue;
                supersets_[k].push_back(i);
                LoopCtlPair pr;
                pr.k = k;
                pr.source_key = c.key;
                pr.group = gid.emplace(std::make_pair(k, c.slam_id), static_cast<int32_t>(gid.size())).first->second;
                loop_math::guess(&new_norm_[size_t(k) * 16], c.estimate, p.use_planar_registration_guess, pr.guess);
                pairs1_.push_back(pr);
            }
        }
        n_groups_ = static_cast<int>(gid.size());
        return true;
    }
    const std::vector<LoopCtlPair>& stage1() const { return pairs1_; }
    int n_groups() const { return n_groups_; }
    // every key the two stages can name besides the stage-1 pairs: the neighbours of the superset candidates the consistency check may reach
    std::vector<uint64_t> possible_consistency_keys() const
    {
        std::vector<uint64_t> out;
        if (!p.enable_consistency_check) return out;
        for (int k = 0; k < n_new_; ++k)
            for (int i : supersets_[k]) {
                const LoopCtlKeyframe& c = kfs_[i];
                if (c.first_keyframe || c.static_keyframe) continue;
                if (c.prev_key) out.push_back(c.prev_key);
                if (c.next_key) out.push_back(c.next_key);
            }
        return out;
    }

    // ---- step 3 + 5: the best match of every subset of gated instances, and its previous / next keyframe against the same target
    const std::vector<LoopCtlPair>& plan_consistency(const LoopCtlRecord* rec1)
    {
        pairs2_.clear();
        std::set<std::pair<int, uint64_t>> seen;
        size_t first = 0;
        for (int k = 0; k < n_new_; ++k) {
            const std::vector<int>& cands = supersets_[k];
            std::vector<uint64_t> robots;
            for (int i : cands) robots.push_back(kfs_[i].slam_id);
            std::sort(robots.begin(), robots.end());
            robots.erase(std::unique(robots.begin(), robots.end()), robots.end());
            auto consider = [&](const std::vector<char>& keep) {
                double best_score;
                const int b = best_of(k, rec1 + first, keep, &best_score);
                const LoopCtlKeyframe* bm = b >= 0 ? &kfs_[cands[b]] : nullptr;
                if (!needs_alignments(bm, best_score)) return;
                for (uint64_t nb : {bm->prev_key, bm->next_key}) {
                    if (nb == 0 || !seen.insert({k, nb}).second) continue;
                    LoopCtlPair pr;
                    pr.k = k;
                    pr.source_key = nb;
                    pr.group = -1;
                    loop_math::guess(&new_norm_[size_t(k) * 16], by_key_.at(nb)->estimate, p.use_planar_registration_guess, pr.guess);
                    pairs2_.push_back(pr);
                }
            };
            std::vector<char> keep(cands.size());
            if (robots.size() <= 12) {  // every subset of gated instances, in the mirror's order
                for (uint32_t mask = 0; mask < (1u << robots.size()); ++mask) {
                    for (size_t c = 0; c < cands.size(); ++c) {
                        const size_t bit = std::lower_bound(robots.begin(), robots.end(), kfs_[cands[c]].slam_id) - robots.begin();
                        keep[c] = !(mask >> bit & 1u);
                    }
                    consider(keep);
                }
            } else {  // the best of a union of instances is the best of one of them: the same set of pairs from the whole list and each instance alone
                std::fill(keep.begin(), keep.end(), 1);
                consider(keep);
                for (uint64_t r : robots) {
                    for (size_t c = 0; c < cands.size(); ++c) keep[c] = kfs_[cands[c]].slam_id == r;
                    consider(keep);
                }
            }
            first += cands.size();
        }
        return pairs2_;
    }

    // ---- step 6 + 7: the reference's loop on the records.  The state changes only when the loops fit `capacity`; returns the number of loops (which
    // may exceed capacity: nothing was written or changed then).
    int replay(const LoopCtlRecord* rec1, const LoopCtlRecord* rec2, double elapsed_us, LoopCtlLoop* out, int capacity)
    {
        State next = state;
        std::map<std::pair<int, uint64_t>, const LoopCtlRecord*> T2;
        for (size_t i = 0; i < pairs2_.size(); ++i) T2[{pairs2_[i].k, pairs2_[i].source_key}] = &rec2[i];
        std::vector<LoopCtlLoop> found;
        std::vector<int32_t> kept_sizes;
        size_t first = 0;
        for (int k = 0; k < n_new_; ++k) {
            const LoopCtlKeyframe& nk = news_[k];
            const std::vector<int>& cands = supersets_[k];
            const LoopCtlRecord* rec = rec1 + first;
            first += cands.size();
            std::vector<char> keep(cands.size());
            int32_t n_cand = 0;
            for (size_t c = 0; c < cands.size(); ++c) { keep[c] = !gate(next, nk, kfs_[cands[c]].slam_id); n_cand += keep[c]; }
            if (n_cand == 0) continue;
            kept_sizes.push_back(n_cand);
            double best_score;
            const int b = best_of(k, rec, keep, &best_score);
            const LoopCtlKeyframe* bm = b >= 0 ? &kfs_[cands[b]] : nullptr;
            bool consistent = false;
            if (bm && (bm->first_keyframe || bm->static_keyframe)) {
                consistent = true;
            } else if (needs_alignments(bm, best_score)) {  // :212-303, the previous keyframe first, the next one only if that failed
                auto pv = bm->prev_key ? T2.find({k, bm->prev_key}) : T2.end();
                auto nx = bm->next_key ? T2.find({k, bm->next_key}) : T2.end();
                consistent = (pv != T2.end() && consistent_prev(*bm, rec[b].T, pv->second->T)) || (nx != T2.end() && consistent_next(*bm, rec[b].T, nx->second->T));
            }
            if (best_score > p.fitness_score_thresh) continue;  // :156-160
            if (!bm) continue;                                  // (nothing converged under a threshold of DBL_MAX: the reference would dereference null)
            if (p.enable_consistency_check && !bm->first_keyframe && !consistent) continue;  // :162-166
            LoopCtlLoop lp;
            lp.key1 = nk.key;
            lp.key2 = bm->key;
            std::memcpy(lp.relative_pose, rec[b].T, sizeof(lp.relative_pose));
            lp.score = best_score;
            found.push_back(lp);
            next.loops[{nk.slam_id, bm->slam_id}] = ManagerEntry{nk.key, bm->key, nk.accum_distance};  // add_loop
        }
        if (static_cast<int>(found.size()) > capacity) return static_cast<int>(found.size());
        // the reference's counters: the candidates the sequential loop would have aligned; the call's time shared out by candidate count
        int64_t total = 0;
        for (int32_t n : kept_sizes) total += n;
        for (int32_t n : kept_sizes) {
            next.candidates_sizes.push_back(n);
            next.detection_times_us.push_back(static_cast<int64_t>(elapsed_us * n / double(total)));
        }
        superset_pairs = static_cast<int64_t>(pairs1_.size());
        sequential_pairs = total;
        consistency_pairs = static_cast<int64_t>(pairs2_.size());
        new_keyframes = n_new_;
        state = std::move(next);
        for (size_t i = 0; i < found.size(); ++i) out[i] = found[i];
        return static_cast<int>(found.size());
    }

    // :77-90, true = the candidates of that instance are skipped: a loop was closed too recently (in accumulated distance) between the two instances
    bool gate(const State& s, const LoopCtlKeyframe& nk, uint64_t cand_slam) const
    {
        auto it = s.loops.find({nk.slam_id, cand_slam});
        if (it == s.loops.end()) return false;
        const double since = nk.accum_distance - it->second.key1_accum_distance;
        if (nk.slam_id == cand_slam) return since < p.accum_distance_thresh_same_robot;
        return since < p.accum_distance_thresh_other_robot;
    }

   private:
    // the rule of :137-144 over the candidates `keep` leaves, in candidate order: the index into the superset, or -1
    int best_of(int k, const LoopCtlRecord* rec, const std::vector<char>& keep, double* best_score) const
    {
        double best = DBL_MAX;
        int    b = -1;
        for (size_t c = 0; c < supersets_[k].size(); ++c) {
            if (!keep[c] || !rec[c].converged || rec[c].fitness > best) continue;
            best = rec[c].fitness;
            b = static_cast<int>(c);
        }
        *best_score = best;
        return b;
    }
    // perform_loop_closure_consistency_check reaches the registration (:190-210)
    bool needs_alignments(const LoopCtlKeyframe* bm, double best_score) const
    {
        return bm && !(bm->first_keyframe || bm->static_keyframe) && p.enable_consistency_check && !(best_score > p.fitness_score_thresh);
    }
    bool within(const float M[16]) const
    {
        const float  dt = std::sqrt(M[12] * M[12] + M[13] * M[13] + M[14] * M[14]);
        const double delta_trans = dt, delta_angle = loop_math::angular_distance_to_identity(M);
        return !(delta_trans > p.consistency_max_delta_trans || delta_angle > p.consistency_max_delta_angle);
    }
    static void to_float(const double in[16], float out[16]) { for (int i = 0; i < 16; ++i) out[i] = static_cast<float>(in[i]); }
    bool consistent_prev(const LoopCtlKeyframe& bm, const float new_to_best[16], const float new_to_prev[16]) const
    {
        float cand_to_prev[16], inv[16], M[16];
        to_float(bm.prev_relpose, cand_to_prev);  // :218
        loop_math::inverse_f(new_to_prev, inv);
        loop_math::mul_f(inv, new_to_best, M);
        loop_math::mul_f(M, cand_to_prev, M);  // :233
        return within(M);
    }
    bool consistent_next(const LoopCtlKeyframe& bm, const float new_to_best[16], const float new_to_next[16]) const
    {
        float next_to_cand[16], inv[16], M[16];
        to_float(bm.next_relpose, next_to_cand);  // :261
        loop_math::inverse_f(new_to_best, inv);
        loop_math::mul_f(inv, new_to_next, M);
        loop_math::mul_f(M, next_to_cand, M);  // :276
        return within(M);
    }
    const LoopCtlKeyframe* kfs_ = nullptr;
    const LoopCtlKeyframe* news_ = nullptr;
    int n_new_ = 0, n_groups_ = 0;
    std::unordered_map<uint64_t, const LoopCtlKeyframe*> by_key_;
    std::vector<std::vector<int>> supersets_;  // per new keyframe: indices into the keyframe list, in list order
    std::vector<double> new_norm_;             // per new keyframe: normalize_estimate(estimate)
    std::vector<LoopCtlPair> pairs1_, pairs2_;
};

}  // namespace mrgfe
