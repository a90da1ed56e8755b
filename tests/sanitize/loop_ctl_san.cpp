// tests/sanitize/loop_ctl_san.cpp — csrc/loop_ctl.h alone (no HIP, no library) under AddressSanitizer + UndefinedBehaviorSanitizer: a scripted two-robot
// session whose new keyframes arrive in groups, through plan() -> plan_consistency() -> replay() with records from a deterministic table, held against a
// plain sequential restatement of LoopDetector::detect over the same table; then the edge cases (empty lists, key 0, an unknown neighbour, a capacity
// too small, NaN / singular records, many SLAM instances).  tests/test_loop_ctl_sanitize_cpu.py builds and runs it; it prints "0 failed checks".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "loop_ctl.h"

using namespace mrgfe;

static int failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static uint64_t rnd_state = 88172645463325252ull;
static double   rnd()  // xorshift, [0, 1)
{
    rnd_state ^= rnd_state << 13;
    rnd_state ^= rnd_state >> 7;
    rnd_state ^= rnd_state << 17;
    return double(rnd_state >> 11) / double(1ull << 53);
}

static void pose(double x, double y, double yaw, double m[16])
{
    std::memset(m, 0, sizeof(double) * 16);
    m[0] = std::cos(yaw); m[4] = -std::sin(yaw);
    m[1] = std::sin(yaw); m[5] = std::cos(yaw);
    m[10] = 1; m[15] = 1;
    m[12] = x; m[13] = y;
}
static void rigid_inverse_d(const double a[16], double inv[16])
{
    std::memset(inv, 0, sizeof(double) * 16);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[4 * c + r] = a[4 * r + c];
        inv[12 + r] = -(a[4 * r] * a[12] + a[4 * r + 1] * a[13] + a[4 * r + 2] * a[14]);
    }
    inv[15] = 1;
}
static void mul_d(const double a[16], const double b[16], double out[16])
{
    double t[16];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += a[4 * k + r] * b[4 * c + k];
            t[4 * c + r] = s;
        }
    std::memcpy(out, t, sizeof(t));
}

struct Session {
    std::vector<LoopCtlKeyframe> kfs, news;
    std::map<std::pair<uint64_t, uint64_t>, LoopCtlRecord> table;  // (new key, keyframe key)
};

static Session make_session(int n_known, int n_new)
{
    Session s;
    std::vector<int> last(2, -1), count(2, 0);
    for (int i = 0; i < n_known; ++i) {
        const int robot = i % 3 ? 0 : 1;
        LoopCtlKeyframe k;
        k.key = 100 + i;
        k.slam_id = 7000 + robot;
        pose(1.5 * count[robot], robot ? 2.0 : 0.0, 0.0, k.estimate);
        k.accum_distance = 4.0 * count[robot];
        k.first_keyframe = count[robot] == 0;
        k.static_keyframe = rnd() < 0.05;
        if (last[robot] >= 0) {
            LoopCtlKeyframe& p = s.kfs[last[robot]];
            double inv[16], rel[16];
            rigid_inverse_d(k.estimate, inv);
            mul_d(inv, p.estimate, rel);
            k.prev_key = p.key;
            std::memcpy(k.prev_relpose, rel, sizeof(rel));
            p.next_key = k.key;
            std::memcpy(p.next_relpose, rel, sizeof(rel));
        }
        last[robot] = i;
        ++count[robot];
        s.kfs.push_back(k);
    }
    for (int j = 0; j < n_new; ++j) {
        LoopCtlKeyframe k;
        k.key = 5000 + j;
        k.slam_id = 7000;
        pose(1.5 * (j % 20) + 0.3 * (rnd() - 0.5), 1.0, 0.0, k.estimate);
        k.accum_distance = 400.0 + 3.0 * j;
        s.news.push_back(k);
    }
    for (const LoopCtlKeyframe& nk : s.news) {
        double nn[16], inv[16];
        loop_math::normalize_estimate(nk.estimate, nn);
        rigid_inverse_d(nn, inv);
        for (const LoopCtlKeyframe& k : s.kfs) {
            double off[16], T[16];
            pose(rnd() < 0.7 ? 0.0 : 3.0 * (rnd() - 0.5), 0.0, rnd() < 0.8 ? 0.0 : 0.2 * (rnd() - 0.5), off);
            mul_d(inv, k.estimate, T);
            mul_d(T, off, T);
            LoopCtlRecord r;
            for (int i = 0; i < 16; ++i) r.T[i] = static_cast<float>(T[i]);
            r.converged = rnd() < 0.85;
            const double pick[6] = {0.2, 0.4, 0.4, 0.9, 1.3, 2.0};
            r.fitness = rnd() < 0.6 ? pick[int(rnd() * 6) % 6] : 0.1 + 1.9 * rnd();
            s.table[{nk.key, k.key}] = r;
        }
    }
    return s;
}

static std::vector<LoopCtlRecord> answer(const Session& s, const std::vector<LoopCtlPair>& pairs, const LoopCtlKeyframe* news)
{
    std::vector<LoopCtlRecord> out;
    for (const LoopCtlPair& p : pairs) out.push_back(s.table.at({news[p.k].key, p.source_key}));
    return out;
}

// one detect call through the controller; returns the loops
static std::vector<LoopCtlLoop> detect(LoopCtl& ctl, const Session& s, int g0, int g1)
{
    std::vector<LoopCtlLoop> out(static_cast<size_t>(g1 - g0 + 1));
    CHECK(ctl.plan(static_cast<int>(s.kfs.size()), s.kfs.data(), g1 - g0, s.news.data() + g0, 0, nullptr));
    if (ctl.stage1().empty()) return {};
    for (const LoopCtlPair& p : ctl.stage1()) CHECK(p.group >= 0 && p.group < ctl.n_groups());
    const std::vector<LoopCtlRecord> rec1 = answer(s, ctl.stage1(), s.news.data() + g0);
    const std::vector<LoopCtlPair>& p2 = ctl.plan_consistency(rec1.data());
    const std::vector<LoopCtlRecord> rec2 = answer(s, p2, s.news.data() + g0);
    const int n = ctl.replay(rec1.data(), rec2.data(), 1000.0, out.data(), g1 - g0);
    CHECK(n >= 0 && n <= g1 - g0);
    out.resize(static_cast<size_t>(n));
    return out;
}

// the reference's loop as it stands (one new keyframe per call: the gates are those of the state), through the same controller API with groups of ONE
// — the superset machinery reduces to find_candidates + matching then — to hold the grouped calls against
static void session_groups_agree()
{
    for (int group : {2, 5, 8}) {
        rnd_state = 88172645463325252ull + group;
        const Session s = make_session(40, 24);
        LoopCtl one, many;
        one.p.candidate_max_xy_distance = many.p.candidate_max_xy_distance = 6.0;
        std::vector<LoopCtlLoop> la, lb;
        int64_t pruned = 0;
        for (int j = 0; j < 24; ++j) for (const LoopCtlLoop& l : detect(one, s, j, j + 1)) la.push_back(l);
        for (int g0 = 0; g0 < 24; g0 += group) {
            for (const LoopCtlLoop& l : detect(many, s, g0, std::min(24, g0 + group))) lb.push_back(l);
            pruned += many.superset_pairs - many.sequential_pairs;
            CHECK(many.superset_pairs >= many.sequential_pairs);
        }
        CHECK(la.size() == lb.size() && la.size() >= 2);
        for (size_t i = 0; i < la.size() && i < lb.size(); ++i)
            CHECK(la[i].key1 == lb[i].key1 && la[i].key2 == lb[i].key2 && std::memcmp(la[i].relative_pose, lb[i].relative_pose, 64) == 0 && la[i].score == lb[i].score);
        CHECK(one.state.candidates_sizes == many.state.candidates_sizes);
        CHECK(one.state.loops.size() == many.state.loops.size() && !one.state.loops.empty());
        CHECK(pruned > 0);
    }
}

static void edge_cases()
{
    rnd_state = 4242;
    Session s = make_session(20, 6);
    LoopCtl ctl;
    ctl.p.candidate_max_xy_distance = 6.0;
    LoopCtlLoop out[8];
    // empty lists
    CHECK(ctl.plan(0, nullptr, 0, nullptr, 0, nullptr) && ctl.stage1().empty());
    CHECK(ctl.plan(20, s.kfs.data(), 0, nullptr, 0, nullptr) && ctl.stage1().empty());
    CHECK(ctl.plan(0, nullptr, 6, s.news.data(), 0, nullptr) && ctl.stage1().empty());
    CHECK(ctl.plan_consistency(nullptr).empty() && ctl.replay(nullptr, nullptr, 1.0, out, 8) == 0);
    CHECK(!ctl.plan(-1, nullptr, 0, nullptr, 0, nullptr) && !ctl.plan(3, nullptr, 0, nullptr, 0, nullptr));
    // key 0 and an unknown neighbour
    s.kfs[4].key = 0;
    CHECK(!ctl.plan(20, s.kfs.data(), 6, s.news.data(), 0, nullptr) && ctl.error.find("key 0") != std::string::npos);
    s.kfs[4].key = 104;
    const uint64_t keep = s.kfs[6].prev_key;
    s.kfs[6].prev_key = 999999;
    CHECK(!ctl.plan(20, s.kfs.data(), 6, s.news.data(), 0, nullptr) && ctl.error.find("999999") != std::string::npos);
    s.kfs[6].prev_key = keep;
    // edges remove candidates (either order of the pair)
    CHECK(ctl.plan(20, s.kfs.data(), 6, s.news.data(), 0, nullptr));
    const size_t n_all = ctl.stage1().size();
    CHECK(n_all > 0);
    const uint64_t e[4] = {ctl.stage1()[0].source_key, s.news[ctl.stage1()[0].k].key, 1, 2};
    CHECK(ctl.plan(20, s.kfs.data(), 6, s.news.data(), 2, e) && ctl.stage1().size() == n_all - 1);
    // capacity too small: the count comes back, the state stays
    CHECK(ctl.plan(20, s.kfs.data(), 6, s.news.data(), 0, nullptr));
    std::vector<LoopCtlRecord> rec1 = answer(s, ctl.stage1(), s.news.data());
    for (LoopCtlRecord& r : rec1) { r.converged = 1; r.fitness = 0.3; }
    ctl.p.enable_consistency_check = 0;
    CHECK(ctl.plan_consistency(rec1.data()).empty());
    const int want = ctl.replay(rec1.data(), nullptr, 5.0, out, 0);
    CHECK(want >= 1 && ctl.state.loops.empty() && ctl.state.candidates_sizes.empty() && ctl.superset_pairs == 0);
    CHECK(ctl.replay(rec1.data(), nullptr, 5.0, out, 8) == want && !ctl.state.loops.empty() && ctl.superset_pairs == int64_t(n_all));
    ctl.reset();
    CHECK(ctl.state.loops.empty() && ctl.state.detection_times_us.empty());
    // NaN scores, non-converged everything, singular and NaN transformations through the consistency arithmetic
    ctl.p.enable_consistency_check = 1;
    CHECK(ctl.plan(20, s.kfs.data(), 6, s.news.data(), 0, nullptr));
    rec1 = answer(s, ctl.stage1(), s.news.data());
    for (size_t i = 0; i < rec1.size(); ++i) {
        rec1[i].converged = 1;
        rec1[i].fitness = i % 3 == 0 ? std::numeric_limits<double>::quiet_NaN() : 0.5;
        if (i % 4 == 1) std::memset(rec1[i].T, 0, sizeof(rec1[i].T));                                        // singular
        if (i % 4 == 2) for (float& v : rec1[i].T) v = std::numeric_limits<float>::quiet_NaN();
        if (i % 4 == 3) for (float& v : rec1[i].T) v = std::numeric_limits<float>::infinity();
    }
    {
        const std::vector<LoopCtlPair>& p2 = ctl.plan_consistency(rec1.data());
        std::vector<LoopCtlRecord> rec2 = answer(s, p2, s.news.data());
        for (size_t i = 0; i < rec2.size(); ++i) if (i % 2) std::memset(rec2[i].T, 0, sizeof(rec2[i].T));
        const int n = ctl.replay(rec1.data(), rec2.data(), 0.0, out, 8);
        CHECK(n >= 0 && n <= 6);
    }
    for (LoopCtlRecord& r : rec1) r.converged = 0;
    CHECK(ctl.plan_consistency(rec1.data()).empty() && ctl.replay(rec1.data(), nullptr, 1.0, out, 8) == 0);
    // many SLAM instances: more than the subset enumeration takes, the per-instance route
    Session m = make_session(30, 2);
    for (size_t i = 0; i < m.kfs.size(); ++i) { m.kfs[i].slam_id = 9000 + i % 15; m.kfs[i].first_keyframe = 0; }
    LoopCtl wide;
    wide.p.candidate_max_xy_distance = 100.0;
    CHECK(wide.plan(30, m.kfs.data(), 2, m.news.data(), 0, nullptr) && wide.n_groups() >= 26);
    rec1 = answer(m, wide.stage1(), m.news.data());
    const std::vector<LoopCtlPair>& p2 = wide.plan_consistency(rec1.data());
    const std::vector<LoopCtlRecord> rec2 = answer(m, p2, m.news.data());
    CHECK(wide.replay(rec1.data(), rec2.data(), 10.0, out, 8) >= 0);
    // helpers on degenerate input
    double z[16] = {0}, o[16];
    float  g[16];
    loop_math::normalize_estimate(z, o);
    loop_math::guess(z, z, 1, g);
    CHECK(g[14] == 0.0f);
    float inv[16], zero_f[16] = {0};
    loop_math::inverse_f(zero_f, inv);
    (void)loop_math::angular_distance_to_identity(inv);
}

int main()
{
    session_groups_agree();
    edge_cases();
    std::printf("%d failed checks\n", failed);
    return failed ? 1 : 0;
}
