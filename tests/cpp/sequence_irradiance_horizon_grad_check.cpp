// sequence_irradiance_horizon_grad_check -- SunskySequence's irradiance gradients under a horizon
// profile (include/sunsky_amd.hpp) in host mode, driven by
// tests/test_sequence_irradiance_horizon_grad_cpp.py: irradiance_horizon_vjp compiles against the
// header and refuses in the places the C ABI does.
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
    const std::vector<float> dirs = {0.9f, 0.f, 0.4f, -0.001f, 0.5f, 0.8f, -1.f, -0.001f, -0.1f};
    const std::vector<float> turb = {2.5f, 6.f, 3.f}, weights = {0.5f, 0.f, 1.f};
    SunskySequence seq(parent, dirs, turb, weights);
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{450.f, 550.f} : std::vector<float>{};

    float buf[64] = {0.f, 0.f, 1.f};
    const Vector3 nrm{buf, buf, buf};
    Vector3Out gn;
    gn.x = gn.y = gn.z = buf;
    auto call = [&](int sectors, bool per_receiver, size_t hstride = 0, size_t ghstride = 0, bool with_gh = true, size_t n = 4) {
        seq.irradiance_horizon_vjp(nrm, n, buf, sectors, per_receiver, buf, gn, buf, with_gh ? buf : nullptr, nullptr, hstride, 0,
                                   ghstride);
    };

    // the strides come before the sequence's state; then the missing preparation is named
    EXPECT(has(error_of([&] { call(0, false); }), "n_sectors"));
    EXPECT(has(error_of([&] { call(4, true, 3); }), "horizon_stride < n"));
    EXPECT(has(error_of([&] { call(4, true, 0, 3); }), "grad_horizon_stride < n"));
    const std::string a = error_of([&] { call(4, true); });
    std::printf("no tables: %s\n", a.c_str());
    EXPECT(has(a, "sunsky_sequence_prepare_irradiance first"));
    seq.prepare_irradiance(8, 16, lam);
    const std::string b = error_of([&] { call(4, true); });
    std::printf("no gradient preparation: %s\n", b.c_str());
    EXPECT(has(b, "sunsky_sequence_prepare_irradiance_grad first"));
    seq.prepare_irradiance_grad();

    const std::string c = error_of([&] { call(3, true); });
    std::printf("3 sectors: %s\n", c.c_str());
    EXPECT(has(c, "n_sectors"));
    EXPECT(has(error_of([&] { call(32, false); }), "n_sectors"));
    EXPECT(has(error_of([&] {
        check(sunsky_sequence_irradiance_horizon_vjp(seq.handle(), sunsky_vec3_in{buf, buf, buf}, buf, 4, 2, 4, nullptr, 4, buf, 4,
                                                     sunsky_vec3_out{buf, buf, buf}, buf, buf, 4, nullptr));
    }), "n_profiles"));
    const std::string d = error_of([&] { call(4, true); });
    std::printf("prepared: %s\n", d.c_str());
    EXPECT(has(d, "host-only sequence"));
    EXPECT(has(error_of([&] { call(4, false); }), "host-only sequence"));
    EXPECT(has(error_of([&] { call(1, true, 1, 1); }), "host-only sequence"));          // one sector: any stride
    EXPECT(has(error_of([&] { call(4, true, 0, 3, false); }), "host-only sequence")); // no grad_horizon: its stride is not looked at
    EXPECT(has(error_of([&] {
        seq.irradiance_horizon_vjp(nrm, 4, buf, 4, true, buf, Vector3Out{}, nullptr, nullptr);
    }), "host-only sequence"));
    EXPECT(has(error_of([&] { seq.irradiance_horizon_vjp(nrm, 4, nullptr, 4, false, buf, gn, buf, buf); }), "null horizon"));
    EXPECT(has(error_of([&] { seq.irradiance_horizon_vjp(nrm, 4, buf, 4, false, nullptr, gn, buf, buf); }), "d_out"));
    seq.irradiance_horizon_vjp(Vector3{}, 0, nullptr, 0, false, nullptr, Vector3Out{}, nullptr, nullptr);   // n == 0 succeeds

    // sticky: new tables restage the preparation; update drops it with the tables
    seq.prepare_irradiance(4, 8, lam);
    EXPECT(has(error_of([&] { call(4, true); }), "host-only sequence"));
    seq.update({}, {}, {1.f, 1.f, 1.f});
    EXPECT(has(error_of([&] { call(4, true); }), "sunsky_sequence_prepare_irradiance first"));
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_irradiance_horizon_grad_check host\n");
        return 2;
    }
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence irradiance horizon grad host ok\n");
    return 0;
}
