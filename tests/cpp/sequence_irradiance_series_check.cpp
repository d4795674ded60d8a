// sequence_irradiance_series_check -- SunskySequence's per-frame irradiance series
// (include/sunsky_amd.hpp) in host mode, driven by tests/test_sequence_irradiance_series_cpp.py:
// prepare_irradiance_series, irradiance_frame_table and irradiance_series compile against the
// header and refuse in the places the C ABI does.
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

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static void host_mode(Variant variant) {
    Properties base;
    base.set_float("turbidity", 4.f).set_float("albedo", 0.2).set_vector3("sun_direction", 0.f, 0.f, 1.f);
    SunskyEmitter parent = SunskyEmitter::host_only(base, variant);
    // the last sun is below the horizon
    const std::vector<float> dirs = {0.9f, 0.f, 0.4f, -0.001f, 0.5f, 0.8f, -1.f, -0.001f, -0.1f};
    const std::vector<float> turb = {2.5f, 6.f, 3.f}, weights = {0.5f, 0.f, 1.f};
    SunskySequence seq(parent, dirs, turb, weights);
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{450.f, 550.f} : std::vector<float>{};
    const size_t planes = variant == Variant::Spectral ? 2 : 3;

    float buf[16] = {0.f, 0.f, 1.f};
    const Vector3 nrm{buf, buf, buf};
    SpectrumOut out;
    out.data = buf;
    out.stride = 4;

    // before anything is prepared: the launch names its own preparation, which names the tables'
    const std::string a = error_of([&] { seq.irradiance_series(nrm, 4, out); });
    std::printf("nothing prepared: %s\n", a.c_str());
    EXPECT(has(a, "sunsky_sequence_prepare_irradiance_series first"));
    EXPECT(has(error_of([&] { seq.prepare_irradiance_series(); }), "sunsky_sequence_prepare_irradiance first"));
    EXPECT(has(error_of([&] { seq.irradiance_frame_table(0); }), "sunsky_sequence_prepare_irradiance first"));

    seq.prepare_irradiance(8, 16, lam);
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out); }), "sunsky_sequence_prepare_irradiance_series first"));
    // a frame's own table needs the tables only: the night frame's is exactly 0, a day frame's is not
    const std::vector<float> day = seq.irradiance_frame_table(1), night = seq.irradiance_frame_table(2);
    EXPECT(day.size() == planes * 8 * 16 && night.size() == day.size());
    float most = 0.f, dark = 0.f;
    for (float v : day) most = v > most ? v : most;
    for (float v : night) dark = v != 0.f ? 1.f : dark;
    EXPECT(most > 0.f && dark == 0.f);
    EXPECT(has(error_of([&] { seq.irradiance_frame_table(3); }), "frame index out of range"));

    seq.prepare_irradiance_series();
    // the header's order: the frame range, the horizon's three, out's stride, then the host-only refusal
    const std::string b = error_of([&] { seq.irradiance_series(nrm, 4, out, 2, 2); });
    std::printf("frames (2, 2) of 3: %s\n", b.c_str());
    EXPECT(has(b, "frame range"));
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, -1, 1); }), "frame range"));
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, 4); }), "frame range"));   // all frames from 4 on: -1
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, 0, -1, nullptr, buf, 3, true); }), "n_sectors"));
    EXPECT(has(error_of([&] {
        check(sunsky_sequence_irradiance_series(seq.handle(), sunsky_vec3_in{buf, buf, buf}, buf, 4, 2, 4, nullptr, 4, 0, 3,
                                                buf, 4, nullptr));
    }), "n_profiles"));
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, 0, -1, nullptr, buf, 4, true, 3); }), "horizon_stride"));
    SpectrumOut narrow = out;
    narrow.stride = 3;
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, narrow); }), "out_stride"));
    const std::string c = error_of([&] { seq.irradiance_series(nrm, 4, out); });
    std::printf("prepared: %s\n", c.c_str());
    EXPECT(has(c, "host-only sequence"));
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, 1, 2); }), "host-only sequence"));
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, 0, -1, nullptr, buf, 4, true); }), "host-only sequence"));
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out, 0, -1, nullptr, buf, 16, false); }), "host-only sequence"));
    seq.irradiance_series(Vector3{}, 0, SpectrumOut{});          // n == 0 succeeds
    seq.irradiance_series(Vector3{}, 4, SpectrumOut{}, 3, 0);    // and so does n_frames == 0

    // sticky across new tables; update drops it with them
    seq.prepare_irradiance(4, 8, lam);
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out); }), "host-only sequence"));
    seq.update({}, {}, {1.f, 1.f, 1.f});
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out); }), "sunsky_sequence_prepare_irradiance_series first"));
    seq.prepare_irradiance(4, 8, lam);
    EXPECT(has(error_of([&] { seq.irradiance_series(nrm, 4, out); }), "host-only sequence"));
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_irradiance_series_check host\n");
        return 2;
    }
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence irradiance series host ok\n");
    return 0;
}
