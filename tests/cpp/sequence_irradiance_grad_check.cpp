// sequence_irradiance_grad_check -- SunskySequence's irradiance gradients (include/sunsky_amd.hpp)
// in host mode, driven by tests/test_sequence_irradiance_grad_cpp.py: prepare_irradiance_grad and
// irradiance_vjp refuse in the places the C ABI does, and the preparation is sticky.
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
    const std::vector<float> dirs = {0.9f, 0.f, 0.4f, -0.3f, 0.5f, 0.8f, 0.f, 1.f, -0.1f};
    const std::vector<float> turb = {2.5f, 6.f, 3.f}, weights = {0.5f, 0.f, 1.f};
    SunskySequence seq(parent, dirs, turb, weights);
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{450.f, 550.f} : std::vector<float>{};

    float buf[8] = {0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const Vector3 nrm{buf, buf, buf};
    Vector3Out gn;
    gn.x = gn.y = gn.z = buf;
    auto vjp = [&] { seq.irradiance_vjp(nrm, 1, buf, gn, buf); };

    // before either preparation: the tables are named, by the call and by the preparation
    const std::string a = error_of(vjp);
    std::printf("no tables: %s\n", a.c_str());
    EXPECT(has(a, "sunsky_sequence_prepare_irradiance first"));
    EXPECT(has(error_of([&] { seq.prepare_irradiance_grad(); }), "sunsky_sequence_prepare_irradiance first"));
    seq.prepare_irradiance(8, 16, lam);
    const std::string b = error_of(vjp);
    std::printf("no gradient preparation: %s\n", b.c_str());
    EXPECT(has(b, "sunsky_sequence_prepare_irradiance_grad first"));

    // prepared, but host-only: the launch is refused; n == 0 succeeds; d_out is required
    seq.prepare_irradiance_grad();
    const std::string c = error_of(vjp);
    std::printf("prepared: %s\n", c.c_str());
    EXPECT(has(c, "host-only sequence"));
    seq.irradiance_vjp(Vector3{}, 0, nullptr, Vector3Out{}, nullptr);
    EXPECT(has(error_of([&] { seq.irradiance_vjp(nrm, 1, nullptr, gn, buf); }), "d_out"));
    EXPECT(has(error_of([&] { seq.irradiance_vjp(nrm, 1, buf, Vector3Out{}, nullptr); }), "host-only sequence"));
    Vector3Out part;
    part.x = buf;
    EXPECT(has(error_of([&] { seq.irradiance_vjp(nrm, 1, buf, part, buf); }), "grad_normal"));

    // sticky across new tables; dropped by update with the tables; prepare_irradiance brings it back
    seq.prepare_irradiance(4, 8, lam);
    EXPECT(has(error_of(vjp), "host-only sequence"));
    seq.update({}, {}, {1.f, 1.f, 1.f});
    EXPECT(has(error_of(vjp), "sunsky_sequence_prepare_irradiance first"));
    seq.prepare_irradiance(4, 8, lam);
    EXPECT(has(error_of(vjp), "host-only sequence"));
    EXPECT(seq.irradiance_info().n_planes == (variant == Variant::Spectral ? 2 : 3));
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_irradiance_grad_check host\n");
        return 2;
    }
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence irradiance grad host ok\n");
    return 0;
}
