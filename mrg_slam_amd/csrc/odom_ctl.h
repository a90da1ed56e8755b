// csrc/odom_ctl.h — the state and the decisions of ScanMatchingOdometryComponent::matching (apps/scan_matching_odometry_component.cpp:195-350) as a
// controller the one-call odometry frame (odometry.cpp) drives: begin_frame() gives the guess of :266, end_frame() takes hasConverged() and
// getFinalTransformation() and makes the decisions of :270-339.  Header-only host code, no HIP: tests/sanitize/odom_ctl_san.cpp compiles it alone, and
// mrgfe_dbg_odom_ctl_* (include/mrgfe_debug.h) step it without a GPU.
//
// Arithmetic (it decides the bits of the guess, and with them the bits of every result).  Matrices are column-major float 4x4, element (r, c) at
// [4 c + r], as in the C ABI.
//   * products: row times column, k = 0..3 ascending, every product and every sum rounded to float, never fused (contract off below);
//     guess = prev_trans * msf_delta (:266), odom = keyframe_pose * trans (:276), the non-converged / rejected return keyframe_pose * prev_trans (:272, :307);
//   * the thresholding delta (:279) is inverse(prev_trans) * trans with the RIGID inverse (R^T, -R^T t) in float, formed as mrgfe_status_poses forms it.
//     The reference's general Matrix4f::inverse() is not restated: the delta feeds the two comparisons of :286 and nothing else, and prev_trans is a
//     registration result (or the identity), so both inverses agree far inside any margin a threshold is chosen with;
//   * a translation is the float norm (x x + y y) + z z, sqrtf, promoted to double (:280, :326);
//   * an angle is rotation_angle of mrg_slam_amd/odometry.py: acosf of the clamped w of Eigen::Quaternionf(R) (quat_w, in float), promoted (:281, :327);
//   * delta_time = stamp - keyframe_stamp in double seconds (:328).
// Comparison operators and the order of effects follow :270-339 line for line, `prev_time_ = stamp` on the REJECTED path (:306) and the counter reset
// (:302, :313) included.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace mrgfe {

enum OdomOutcome : int32_t { ODOM_FIRST_FRAME = 0, ODOM_ACCEPTED = 1, ODOM_NOT_CONVERGED = 2, ODOM_REJECTED = 3, ODOM_REJECTED_RESET = 4 };

struct OdomCtlParams {
    double keyframe_delta_translation = 1.0, keyframe_delta_angle = 0.5236, keyframe_delta_time = 10000.0;  // config/mrg_slam.yaml:77-86
    int    enable_transform_thresholding = 0, max_consecutive_rejections = 5;
    double max_acceptable_translation = 1.0, max_acceptable_angle = 1.0;
};

// everything matching() keeps between frames (a plain record: tests compare it byte for byte)
struct OdomCtlState {
    int32_t has_keyframe;            // keyframe_cloud_ != nullptr
    int32_t consecutive_rejections;  // :287, :302, :313
    int32_t has_prev_time;           // prev_time_ != rclcpp::Time() (:198 resets it)
    int32_t reserved;
    double  keyframe_stamp, prev_time;
    float   keyframe_pose[16], prev_trans[16];
};

struct OdomDecision {
    int32_t outcome, new_keyframe, consecutive_rejections;
    float   odom[16];           // what matching() returns
    float   keyframe_pose[16];  // keyframe_pose_ as :323 reads it: before a switch made by this frame
    float   trans[16];          // getFinalTransformation() as given; the identity on the first frame
};

// (every intermediate goes through a volatile float: one rounding per operation whatever the compiler's contraction default is — the library is built
// with -ffp-contract=off, the stand-alone sanitizer program with a host compiler's defaults)
namespace odom_math {
inline void identity(float m[16]) { for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
inline void mul(const float a[16], const float b[16], float out[16])
{
    float t[16];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            volatile float s = a[r] * b[4 * c];  // (volatile: one rounding per operation whatever the compiler's contraction default is)
            for (int k = 1; k < 4; ++k) {
                volatile float p = a[4 * k + r] * b[4 * c + k];
                s = s + p;
            }
            t[4 * c + r] = s;
        }
    std::memcpy(out, t, sizeof(t));
}
// (R^T, -R^T t): the rows of the inverse's rotation are the columns of R; the translation's three-term sums left to right (api.cpp mrgfe_status_poses)
inline void rigid_inverse(const float m[16], float out[16])
{
    float t[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) t[4 * c + r] = m[4 * r + c];
        volatile float p0 = (-m[4 * r + 0]) * m[12], p1 = (-m[4 * r + 1]) * m[13], p2 = (-m[4 * r + 2]) * m[14];
        volatile float s = p0 + p1;
        s = s + p2;
        t[12 + r] = s;
        t[4 * r + 3] = 0.0f;
    }
    t[15] = 1.0f;
    std::memcpy(out, t, sizeof(t));
}
inline double translation_norm(const float m[16])
{
    volatile float xx = m[12] * m[12], yy = m[13] * m[13], zz = m[14] * m[14];
    volatile float s = xx + yy;
    s = s + zz;
    return static_cast<double>(std::sqrt(static_cast<float>(s)));
}
// w of Eigen::Quaternionf(R) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl for a 3 x 3 matrix), in float: odometry.quat_w
inline float quat_w(const float m[16])
{
    auto R = [&](int r, int c) { return m[4 * c + r]; };
    volatile float t = R(0, 0) + R(1, 1);
    t = t + R(2, 2);
    if (t > 0.0f) {
        volatile float u = t + 1.0f;
        return 0.5f * std::sqrt(static_cast<float>(u));
    }
    int i = 0;
    if (R(1, 1) > R(0, 0)) i = 1;
    if (R(2, 2) > R(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    volatile float u = R(i, i) - R(j, j);
    u = u - R(k, k);
    u = u + 1.0f;
    const float tt = std::sqrt(static_cast<float>(u));
    volatile float d = R(k, j) - R(j, k);
    volatile float h = 0.5f / tt;
    return d * h;
}
// odometry.rotation_angle: acos of w clamped to [-1, 1] (a NaN becomes -1, as Python's min / max leave it), in float, promoted
inline double rotation_angle(const float m[16])
{
    float w = quat_w(m);
    w = w > -1.0f ? w : -1.0f;
    w = w < 1.0f ? w : 1.0f;
    return static_cast<double>(std::acos(w));
}
}  // namespace odom_math

class OdomController {
   public:
    OdomController() { reset(); }
    explicit OdomController(const OdomCtlParams& p) : prm_(p) { reset(); }
    // forgets the keyframe: the next frame is a first frame (:197-205)
    void reset()
    {
        std::memset(&st_, 0, sizeof(st_));
        odom_math::identity(st_.keyframe_pose);
        odom_math::identity(st_.prev_trans);
        pending_ = false;
    }
    const OdomCtlState&  state() const { return st_; }
    const OdomCtlParams& params() const { return prm_; }
    bool has_keyframe() const { return st_.has_keyframe != 0; }
    bool pending() const { return pending_; }

    // The frame's stamp and prediction (msf_delta column-major, NULL = the identity of :211).  Returns true when the frame is to be aligned, from `guess`
    // = prev_trans * msf_delta (:266); false on a first frame (guess = the identity).  Changes nothing matching() keeps: a frame that fails between
    // begin_frame and end_frame leaves the state as it was.
    bool begin_frame(double stamp, const float* msf_delta, float guess[16])
    {
        pending_ = true;
        pending_stamp_ = stamp;
        if (!st_.has_keyframe) { odom_math::identity(guess); return false; }
        float delta[16];
        if (msf_delta) std::memcpy(delta, msf_delta, sizeof(delta));
        else odom_math::identity(delta);
        odom_math::mul(st_.prev_trans, delta, guess);
        return true;
    }

    // hasConverged() and getFinalTransformation() of the frame begun (both ignored on a first frame; `final` may then be NULL): :197-205, :270-339
    OdomDecision end_frame(bool converged, const float* final)
    {
        using namespace odom_math;
        const double stamp = pending_stamp_;
        pending_ = false;
        OdomDecision d;
        std::memset(&d, 0, sizeof(d));
        if (!st_.has_keyframe) {  // :197-205
            st_.has_prev_time = 0;
            st_.prev_time = 0.0;
            identity(st_.prev_trans);
            identity(st_.keyframe_pose);
            st_.keyframe_stamp = stamp;
            st_.has_keyframe = 1;
            d.outcome = ODOM_FIRST_FRAME;
            d.new_keyframe = 1;
            d.consecutive_rejections = st_.consecutive_rejections;
            identity(d.odom); identity(d.keyframe_pose); identity(d.trans);
            return d;
        }
        std::memcpy(d.keyframe_pose, st_.keyframe_pose, sizeof(d.keyframe_pose));
        if (final) std::memcpy(d.trans, final, sizeof(d.trans));
        else identity(d.trans);
        if (!converged) {  // :270-273
            mul(st_.keyframe_pose, st_.prev_trans, d.odom);
            d.outcome = ODOM_NOT_CONVERGED;
            d.consecutive_rejections = st_.consecutive_rejections;
            return d;
        }
        const float* trans = d.trans;  // :275
        float odom[16];
        mul(st_.keyframe_pose, trans, odom);  // :276
        if (prm_.enable_transform_thresholding) {  // :278
            float inv[16], delta[16];
            rigid_inverse(st_.prev_trans, inv);
            mul(inv, trans, delta);  // :279
            const double dx = translation_norm(delta);  // :280
            const double da = rotation_angle(delta);    // :281
            if (dx > prm_.max_acceptable_translation || da > prm_.max_acceptable_angle) {  // :286
                st_.consecutive_rejections++;  // :287
                if (st_.consecutive_rejections >= prm_.max_consecutive_rejections) {  // :291
                    new_keyframe(odom, stamp);  // :294-301
                    st_.consecutive_rejections = 0;  // :302
                    std::memcpy(d.odom, st_.keyframe_pose, sizeof(d.odom));  // :303
                    d.outcome = ODOM_REJECTED_RESET;
                    d.new_keyframe = 1;
                    d.consecutive_rejections = 0;
                    return d;
                }
                st_.prev_time = stamp;  // :306
                st_.has_prev_time = 1;
                mul(st_.keyframe_pose, st_.prev_trans, d.odom);  // :307
                d.outcome = ODOM_REJECTED;
                d.consecutive_rejections = st_.consecutive_rejections;
                return d;
            }
            st_.consecutive_rejections = 0;  // :313
        }
        st_.prev_time = stamp;  // :317
        st_.has_prev_time = 1;
        std::memcpy(st_.prev_trans, trans, sizeof(st_.prev_trans));  // :318
        const double delta_translation = translation_norm(trans);  // :326
        const double delta_angle = rotation_angle(trans);          // :327
        const double delta_time = stamp - st_.keyframe_stamp;      // :328
        if (delta_translation > prm_.keyframe_delta_translation || delta_angle > prm_.keyframe_delta_angle || delta_time > prm_.keyframe_delta_time) {  // :329-331
            new_keyframe(odom, stamp);  // :332-338
            d.new_keyframe = 1;
        }
        std::memcpy(d.odom, odom, sizeof(d.odom));  // :349
        d.outcome = ODOM_ACCEPTED;
        d.consecutive_rejections = st_.consecutive_rejections;
        return d;
    }

   private:
    void new_keyframe(const float odom[16], double stamp)
    {
        std::memcpy(st_.keyframe_pose, odom, sizeof(st_.keyframe_pose));
        st_.keyframe_stamp = stamp;
        st_.prev_time = stamp;
        st_.has_prev_time = 1;
        odom_math::identity(st_.prev_trans);
    }
    OdomCtlParams prm_;
    OdomCtlState  st_;
    bool          pending_ = false;
    double        pending_stamp_ = 0.0;
};

}  // namespace mrgfe
