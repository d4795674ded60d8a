// sequence_grad_check -- SunskySequence's gradient and update calls (include/sunsky_amd.hpp) in
// host mode, driven by tests/test_sequence_grad_cpp.py: update against a new sequence,
// prepare_grad and frame_tangent on a host-only sequence, and the refusal texts.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sunsky_amd.hpp"

using namespace sunsky_amd;

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static void push_sun(std::vector<float>& dirs, float elevation_deg, float azimuth_deg, float length = 1.f) {
    const float e = elevation_deg * 3.14159265f / 180.f, a = azimuth_deg * 3.14159265f / 180.f;
    dirs.push_back(length * std::cos(e) * std::cos(a));
    dirs.push_back(length * std::cos(e) * std::sin(a));
    dirs.push_back(length * std::sin(e));
}

template <typename F>
static std::string error_of(F&& f) {
    try {
        f();
    } catch (const Error& e) {
        EXPECT(e.status == SUNSKY_ERROR_INVALID_VALUE);
        return e.what();
    }
    return "";
}

static bool same_frame(const SunskySequence::Frame& a, const SunskySequence::Frame& b) {
    return std::memcmp(a.sun_dir_local, b.sun_dir_local, sizeof(a.sun_dir_local)) == 0 && a.weight == b.weight &&
           a.turbidity == b.turbidity && a.sky_params == b.sky_params && a.sky_radiance == b.sky_radiance;
}

static void host_mode(Variant variant) {
    Properties base;
    base.set_float("turbidity", 4.f).set_float("albedo", 0.2).set_vector3("sun_direction", 0.f, 0.f, 1.f);
    SunskyEmitter parent = SunskyEmitter::host_only(base, variant);
    const int nch = variant == Variant::Spectral ? 11 : 3;
    std::vector<float> dirs, other;
    push_sun(dirs, 20.f, 0.f);
    push_sun(dirs, 60.f, 120.f);
    push_sun(dirs, -5.f, 240.f);
    push_sun(other, 35.f, 10.f);
    push_sun(other, 5.f, 200.f);
    push_sun(other, 80.f, 300.f);
    const std::vector<float> turb = {2.5f, 6.f, 3.f}, weights = {0.5f, 2.f, 1.f};
    SunskySequence seq(parent, other, {}, {});
    SunskySequence fresh(parent, dirs, turb, weights);

    float dummy[4] = {0.f, 0.f, 1.f, 0.f};
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{550.f} : std::vector<float>{};
    // before prepare_grad: the message names the missing call
    const std::string a = error_of([&] { seq.frame_tangent(0); });
    std::printf("unprepared: %s\n", a.c_str());
    EXPECT(a.find("sunsky_sequence_prepare_grad first") != std::string::npos);
    EXPECT(error_of([&] { seq.eval_vjp(Vector3{dummy, dummy, dummy}, 1, dummy, dummy, dummy, dummy, lam); })
               .find("sunsky_sequence_prepare_grad first") != std::string::npos);

    // update: the new sequence's bits; a refused update changes nothing; a partial one keeps the rest
    seq.update(dirs, turb, weights);
    for (int k = 0; k < 3; ++k) EXPECT(same_frame(seq.frame(k), fresh.frame(k)));
    const std::string r = error_of([&] { seq.update({}, {2.f, 11.f, 3.f}, {}); });
    std::printf("refused: %s\n", r.c_str());
    EXPECT(r.find("Turbidity value 11.000000 is out of range [1, 10] (frame 1)") != std::string::npos);
    EXPECT(error_of([&] { seq.update({}, {}, {1.f, -1.f, 1.f}); }).find("weight must be finite and >= 0") != std::string::npos);
    EXPECT(error_of([&] { seq.update({1.f, 0.f}, {}, {}); }).find("frame count") != std::string::npos);
    for (int k = 0; k < 3; ++k) EXPECT(same_frame(seq.frame(k), fresh.frame(k)));
    seq.prepare_sampling(8, 16);
    seq.update({}, {}, {1.f, 1.f, 1.f});
    EXPECT(seq.frame(1).weight == 1.f && seq.frame(1).turbidity == 6.f);
    EXPECT(error_of([&] { seq.sampling_info(); }).find("sunsky_sequence_prepare_sampling first") != std::string::npos);
    seq.update({}, {}, weights);

    // gradient records: sizes, a sun below the horizon, the update restages them
    seq.prepare_grad();
    fresh.prepare_grad();
    for (int k = 0; k < 3; ++k) {
        const SunskySequence::FrameTangent t = seq.frame_tangent(k), u = fresh.frame_tangent(k);
        EXPECT((int)t.dsky_turbidity.size() == nch * 10 && (int)t.dsky_elevation.size() == nch * 10);
        EXPECT(t.dsky_turbidity == u.dsky_turbidity && t.dsky_elevation == u.dsky_elevation);
        EXPECT(std::memcmp(t.dsun_local, u.dsun_local, sizeof(t.dsun_local)) == 0);
        double mag = 0.0;
        for (float v : t.dsky_turbidity) mag += std::fabs(v);
        for (float v : t.dsky_elevation) mag += std::fabs(v);
        EXPECT((mag > 0.0) == (k != 2));   // the third sun is below the horizon: zero sky tangents
        // an identity to_world: d local / d s is the projector (I - s s^T), symmetric, s in its null space
        for (int i = 0; i < 3; ++i) {
            double along = 0.0;
            for (int j = 0; j < 3; ++j) {
                EXPECT(std::fabs(t.dsun_local[3 * i + j] - t.dsun_local[3 * j + i]) <= 1e-6f);
                along += (double)t.dsun_local[3 * i + j] * dirs[3 * k + j];
            }
            EXPECT(std::fabs(along) <= 1e-6);
        }
    }
    seq.update(other, {}, {});
    SunskySequence moved(parent, other, turb, weights);
    moved.prepare_grad();
    EXPECT(seq.frame_tangent(0).dsky_turbidity == moved.frame_tangent(0).dsky_turbidity);
    EXPECT(seq.frame_tangent(1).dsky_elevation == moved.frame_tangent(1).dsky_elevation);

    // prepared, but host-only: the batch call still needs a device; a null cotangent is refused first
    EXPECT(error_of([&] { seq.eval_vjp(Vector3{dummy, dummy, dummy}, 1, dummy, dummy, dummy, dummy, lam); })
               .find("host-only sequence") != std::string::npos);
    EXPECT(error_of([&] { seq.eval_vjp(Vector3{dummy, dummy, dummy}, 1, nullptr, dummy, dummy, dummy, lam); })
               .find("null cotangent") != std::string::npos);
    seq.eval_vjp(Vector3{dummy, dummy, dummy}, 0, nullptr, dummy, dummy, dummy, lam);   // n == 0 succeeds
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_grad_check host\n");
        return 2;
    }
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence grad host ok\n");
    return 0;
}
