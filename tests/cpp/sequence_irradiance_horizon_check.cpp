// sequence_irradiance_horizon_check -- SunskySequence's irradiance under a horizon profile
// (include/sunsky_amd.hpp) in host mode, driven by tests/test_sequence_irradiance_horizon_cpp.py:
// irradiance_horizon and irradiance_sun_columns compile against the header and refuse in the
// places the C ABI does.
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
    // suns at azimuth 0 and just past 90 and 180 degrees; the last one below the horizon
    const std::vector<float> dirs = {0.9f, 0.f, 0.4f, -0.001f, 0.5f, 0.8f, -1.f, -0.001f, -0.1f};
    const std::vector<float> turb = {2.5f, 6.f, 3.f}, weights = {0.5f, 0.f, 1.f};
    SunskySequence seq(parent, dirs, turb, weights);
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{450.f, 550.f} : std::vector<float>{};

    float buf[16] = {0.f, 0.f, 1.f};
    const Vector3 nrm{buf, buf, buf};
    SpectrumOut out;
    out.data = buf;
    out.stride = 4;
    auto call = [&](int sectors, bool per_receiver, size_t hstride = 0, size_t n = 4) {
        seq.irradiance_horizon(nrm, n, buf, sectors, per_receiver, out, nullptr, hstride);
    };

    // before prepare_irradiance: the launch and the getter name the missing call
    const std::string a = error_of([&] { call(4, true); });
    std::printf("no tables: %s\n", a.c_str());
    EXPECT(has(a, "sunsky_sequence_prepare_irradiance first"));
    EXPECT(has(error_of([&] { seq.irradiance_sun_columns(); }), "sunsky_sequence_prepare_irradiance first"));

    seq.prepare_irradiance(8, 16, lam);
    const std::vector<int> cols = seq.irradiance_sun_columns();
    EXPECT(cols.size() == 3);
    EXPECT(cols.size() == 3 && cols[0] == 0 && cols[1] == 4 && cols[2] == 8);

    // the header's order: sectors, profiles, the horizon's stride, then the host-only refusal
    const std::string b = error_of([&] { call(3, true); });
    std::printf("3 sectors: %s\n", b.c_str());
    EXPECT(has(b, "n_sectors"));
    EXPECT(has(error_of([&] { call(0, false); }), "n_sectors"));
    EXPECT(has(error_of([&] { call(32, false); }), "n_sectors"));
    EXPECT(has(error_of([&] {
        check(sunsky_sequence_irradiance_horizon(seq.handle(), sunsky_vec3_in{buf, buf, buf}, buf, 4, 2, 4, nullptr, 4,
                                                 buf, 4, nullptr));
    }), "n_profiles"));
    EXPECT(has(error_of([&] { call(4, true, 3); }), "horizon_stride"));
    const std::string c = error_of([&] { call(4, true); });
    std::printf("prepared: %s\n", c.c_str());
    EXPECT(has(c, "host-only sequence"));
    EXPECT(has(error_of([&] { call(4, false); }), "host-only sequence"));
    EXPECT(has(error_of([&] { call(1, true, 1); }), "host-only sequence"));   // one sector: any stride
    EXPECT(has(error_of([&] { seq.irradiance_horizon(nrm, 4, nullptr, 4, false, out); }), "null horizon"));
    seq.irradiance_horizon(Vector3{}, 0, nullptr, 0, false, SpectrumOut{});   // n == 0 succeeds

    // update drops the columns with the tables
    seq.update({}, {}, {1.f, 1.f, 1.f});
    EXPECT(has(error_of([&] { seq.irradiance_sun_columns(); }), "sunsky_sequence_prepare_irradiance first"));
    seq.prepare_irradiance(4, 8, lam);
    EXPECT(seq.irradiance_sun_columns() == (std::vector<int>{0, 2, 4}));
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_irradiance_horizon_check host\n");
        return 2;
    }
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence irradiance horizon host ok\n");
    return 0;
}
