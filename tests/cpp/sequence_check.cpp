// sequence_check -- the SunskySequence facade (include/sunsky_amd.hpp) in host mode, driven by
// tests/test_sequence_cpp.py: frames staged on the host against single host emitters, the
// error mapping, RAII moves and the refusal of batch calls without a device.
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

static std::vector<float> sun_at(float elevation_deg, float azimuth_deg) {
    const float e = elevation_deg * 3.14159265f / 180.f, a = azimuth_deg * 3.14159265f / 180.f;
    return {std::cos(e) * std::cos(a), std::cos(e) * std::sin(a), std::sin(e)};
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

static int host_mode(Variant variant) {
    const float elev[3] = {20.f, 60.f, -5.f}, turb[3] = {2.5f, 6.f, 3.f}, wts[3] = {0.5f, 2.f, 1.f};
    Properties base;
    base.set_float("turbidity", 4.f).set_float("albedo", 0.2).set_vector3("sun_direction", 0.f, 0.f, 1.f);
    SunskyEmitter parent = SunskyEmitter::host_only(base, variant);
    std::vector<float> dirs, turbidity(turb, turb + 3), weights(wts, wts + 3);
    for (int k = 0; k < 3; ++k) {
        // unnormalised on purpose: the sequence normalises like the emitter's constructor
        std::vector<float> d = sun_at(elev[k], 30.f * (float)k);
        for (float v : d) dirs.push_back(2.f * v);
    }
    SunskySequence seq(parent, dirs, turbidity, weights);
    const sunsky_sequence_desc info = seq.info();
    EXPECT(info.count == 3 && seq.count() == 3);
    EXPECT(info.variant == (int)variant && info.device == -1);
    EXPECT(info.nb_channels == (variant == Variant::RGB ? 3 : 11));
    for (int k = 0; k < 3; ++k) {
        Properties p;
        p.set_float("turbidity", turb[k]).set_float("albedo", 0.2)
            .set_vector3("sun_direction", dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
        SunskyEmitter single = SunskyEmitter::host_only(p, variant);
        const SunskySequence::Frame f = seq.frame(k);
        EXPECT(f.weight == wts[k] && f.turbidity == turb[k]);
        EXPECT(f.sky_params == single.table(SUNSKY_TABLE_SKY_PARAMS));
        EXPECT(f.sky_radiance == single.table(SUNSKY_TABLE_SKY_RADIANCE));
        const sunsky_info si = single.info();
        EXPECT(std::memcmp(f.sun_dir_local, si.sun_dir_local, sizeof(f.sun_dir_local)) == 0);
        if (elev[k] < 0.f)
            for (float v : f.sky_params) EXPECT(v == 0.f);
    }
    // defaults: the emitter's turbidity, weight 1
    SunskySequence plain(parent, sun_at(45.f, 0.f));
    EXPECT(plain.frame(0).turbidity == 4.f && plain.frame(0).weight == 1.f);
    // RAII: a moved-from sequence owns nothing, the target keeps the frames
    SunskySequence moved(std::move(plain));
    EXPECT(plain.handle() == nullptr && moved.count() == 1);
    plain = std::move(moved);
    EXPECT(moved.handle() == nullptr && plain.count() == 1);
    // validation, with the reference's message where it has one
    const std::string m = error_of([&] { SunskySequence s(parent, sun_at(45.f, 0.f), {12.f}); });
    std::printf("turbidity error: %s\n", m.c_str());
    EXPECT(m.find("Turbidity value 12.000000 is out of range [1, 10]") != std::string::npos);
    EXPECT(!error_of([&] { SunskySequence s(parent, {}); }).empty());
    EXPECT(!error_of([&] { SunskySequence s(parent, {0.f, 0.f, 0.f}); }).empty());
    EXPECT(!error_of([&] { SunskySequence s(parent, sun_at(45.f, 0.f), {}, {-1.f}); }).empty());
    EXPECT(!error_of([&] { SunskySequence s(parent, sun_at(45.f, 0.f), {}, {NAN}); }).empty());
    EXPECT(!error_of([&] { SunskySequence s(parent, {0.f, 1.f}); }).empty());
    // batch calls need a device
    float dummy[4] = {0.f, 0.f, 1.f, 0.f};
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{550.f} : std::vector<float>{};
    const std::string b = error_of([&] { seq.eval(Vector3{dummy, dummy, dummy}, 1, SpectrumOut{dummy, 1}, lam); });
    EXPECT(b.find("host-only sequence") != std::string::npos);
    const std::string c = error_of([&] { seq.bake_latlong(2, 2, 0.f, 1.f, 0.f, 1.f, SpectrumOut{dummy, 4}, lam); });
    EXPECT(c.find("host-only sequence") != std::string::npos);
    return failures;
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_check host\n");
        return 2;
    }
    // sun_coordinates: the emitter's own time/location staging
    Properties tl;
    tl.set_float("hour", 11.5).set_int("month", 3);
    SunskyEmitter timed = SunskyEmitter::host_only(tl, Variant::RGB);
    const SunPosition s = sun_coordinates(2010, 3, 10, 11.5f, 0.f, 0.f, 35.6894f, 139.6917f, 9.f);
    const sunsky_info ti = timed.info();
    EXPECT(s.x == ti.sun_dir_world[0] && s.y == ti.sun_dir_world[1] && s.z == ti.sun_dir_world[2]);
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence host ok\n");
    return 0;
}
