// tests/sanitize/odom_ctl_san.cpp — csrc/odom_ctl.h (the state machine of the one-call odometry frame) alone, for g++ -fsanitize=address,undefined:
// scripted sequences through every branch of matching() (first frame, not converged, keyframe by translation / angle / time, rejected, the rejection
// that resets, accepted after rejections, thresholding off), frames begun and never ended, resets, and NaN / inf / non-rigid final matrices.
// Prints "<n> failed checks"; tests/test_odom_controller_cpu.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "odom_ctl.h"

using namespace mrgfe;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { ++g_failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

// column-major rigid transform: rotation about z by `a`, then about x by `b`, translation t
static void rigid(float a, float b, float tx, float ty, float tz, float m[16])
{
    const float ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b);
    const float Rz[9] = {ca, -sa, 0, sa, ca, 0, 0, 0, 1}, Rx[9] = {1, 0, 0, 0, cb, -sb, 0, sb, cb};
    odom_math::identity(m);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            float s = 0;
            for (int k = 0; k < 3; ++k) s += Rz[3 * r + k] * Rx[3 * k + c];
            m[4 * c + r] = s;
        }
    m[12] = tx; m[13] = ty; m[14] = tz;
}

static bool finite16(const float m[16])
{
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}

int main()
{
    int reached[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // outcomes 0..4, 5 keyframe by switch on ACCEPTED, 6 accepted after rejections, 7 thresholding off
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    for (int seq = 0; seq < 400; ++seq) {
        OdomCtlParams p;
        p.enable_transform_thresholding = seq % 3 != 0;
        p.max_consecutive_rejections = 1 + seq % 4;
        p.max_acceptable_translation = 0.8;
        p.max_acceptable_angle = 0.4;
        p.keyframe_delta_translation = 0.7;
        p.keyframe_delta_angle = 0.3;
        p.keyframe_delta_time = 2.5;
        OdomController c(p);
        int rejections_before = 0;
        for (int f = 0; f < 14; ++f) {
            const double stamp = 100.0 + 0.4 * f;
            float delta[16], guess[16], final[16];
            rigid(0.05f * u(rng), 0.02f * u(rng), 0.1f * u(rng), 0.1f * u(rng), 0.0f, delta);
            const OdomCtlState before = c.state();
            const bool aligns = c.begin_frame(stamp, (f & 1) ? delta : nullptr, guess);
            CHECK(std::memcmp(&before, &c.state(), sizeof(before)) == 0);  // begin_frame changes nothing matching() keeps
            CHECK(aligns == (before.has_keyframe != 0));
            CHECK(finite16(guess));
            if (f % 5 == 3) continue;  // a failed frame: begun, never ended
            const float jump = (f % 4 == 2) ? 3.0f : 0.3f;  // every fourth frame jumps
            rigid(0.2f * u(rng) * jump, 0.05f * u(rng), 0.4f * u(rng) * jump, 0.3f * u(rng), 0.05f * u(rng), final);
            const bool converged = (seq + f) % 7 != 0;
            const OdomDecision d = c.end_frame(converged, aligns ? final : nullptr);
            CHECK(d.outcome >= 0 && d.outcome <= 4);
            reached[d.outcome]++;
            CHECK(finite16(d.odom) && finite16(d.keyframe_pose));
            CHECK((d.outcome == ODOM_FIRST_FRAME) == !aligns);
            if (aligns && !converged) CHECK(d.outcome == ODOM_NOT_CONVERGED && !d.new_keyframe);
            if (d.outcome == ODOM_REJECTED_RESET || d.outcome == ODOM_FIRST_FRAME) CHECK(d.new_keyframe == 1);
            if (d.outcome == ODOM_REJECTED) CHECK(d.consecutive_rejections == rejections_before + 1 && d.consecutive_rejections < p.max_consecutive_rejections);
            if (d.outcome == ODOM_REJECTED || d.outcome == ODOM_REJECTED_RESET) CHECK(p.enable_transform_thresholding);
            if (d.outcome == ODOM_ACCEPTED) {
                if (d.new_keyframe) reached[5]++;
                if (rejections_before > 0) reached[6]++;
                if (!p.enable_transform_thresholding) reached[7]++;
                CHECK(d.consecutive_rejections == (p.enable_transform_thresholding ? 0 : rejections_before));
            }
            if (d.new_keyframe) {
                float id[16];
                odom_math::identity(id);
                CHECK(std::memcmp(c.state().prev_trans, id, sizeof(id)) == 0);
                CHECK(c.state().keyframe_stamp == stamp);
                CHECK(std::memcmp(c.state().keyframe_pose, d.odom, sizeof(id)) == 0);
            }
            CHECK(c.state().consecutive_rejections == d.consecutive_rejections);
            rejections_before = d.consecutive_rejections;
        }
        c.reset();
        CHECK(!c.has_keyframe() && c.state().consecutive_rejections == 0);
    }
    for (int k = 0; k < 8; ++k) CHECK(reached[k] > 0);

    // final matrices no registration should return: NaN, inf, all zero, a scaled / sheared "rotation", huge entries — no decision may trip a sanitizer,
    // and each one is some outcome of the five
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity(), big = std::numeric_limits<float>::max();
    std::vector<std::vector<float>> odd;
    odd.push_back(std::vector<float>(16, nan));
    odd.push_back(std::vector<float>(16, inf));
    odd.push_back(std::vector<float>(16, -inf));
    odd.push_back(std::vector<float>(16, 0.0f));
    odd.push_back(std::vector<float>(16, big));
    odd.push_back({-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, nan, 0, 0, 1});     // trace -3: the else branch of quat_w
    odd.push_back({3, 1, 0, 0, 0, -2, 5, 0, 7, 0, 0.5f, 0, 1e30f, -1e30f, 0, 1});  // sheared and scaled
    odd.push_back({-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1});        // a half turn about y: w == 0
    odd.push_back({1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1});        // about x
    odd.push_back({-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1});        // about z
    for (int thresholding = 0; thresholding < 2; ++thresholding)
        for (size_t i = 0; i < odd.size(); ++i)
            for (size_t j = 0; j < odd.size(); ++j) {
                OdomCtlParams p;
                p.enable_transform_thresholding = thresholding;
                p.max_consecutive_rejections = 2;
                OdomController c(p);
                float guess[16];
                c.begin_frame(0.0, nullptr, guess);
                c.end_frame(false, nullptr);
                // first the odd matrix i is accepted or rejected, then j meets whatever prev_trans / keyframe_pose that left (the rigid inverse of an odd matrix)
                for (const std::vector<float>* m : {&odd[i], &odd[j], &odd[j]}) {
                    c.begin_frame(1.0, (i & 1) ? odd[j].data() : nullptr, guess);
                    const OdomDecision d = c.end_frame(true, m->data());
                    CHECK(d.outcome >= 1 && d.outcome <= 4);
                }
                c.begin_frame(std::numeric_limits<double>::quiet_NaN(), nullptr, guess);
                const OdomDecision d = c.end_frame(true, odd[i].data());
                CHECK(d.outcome >= 1 && d.outcome <= 4);
            }
    std::printf("%d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
