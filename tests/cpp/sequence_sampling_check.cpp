// sequence_sampling_check -- SunskySequence's sampling calls (include/sunsky_amd.hpp) in host
// mode, driven by tests/test_sequence_sampling_cpp.py: prepare_sampling and the read-backs on a
// host-only sequence, the derived scalars, and the refusal texts.
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

static void push_sun(std::vector<float>& dirs, float elevation_deg, float azimuth_deg) {
    const float e = elevation_deg * 3.14159265f / 180.f, a = azimuth_deg * 3.14159265f / 180.f;
    dirs.push_back(std::cos(e) * std::cos(a));
    dirs.push_back(std::cos(e) * std::sin(a));
    dirs.push_back(std::sin(e));
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

static void host_mode(Variant variant) {
    Properties base;
    base.set_float("turbidity", 4.f).set_float("albedo", 0.2).set_vector3("sun_direction", 0.f, 0.f, 1.f);
    SunskyEmitter parent = SunskyEmitter::host_only(base, variant);
    std::vector<float> dirs;
    push_sun(dirs, 20.f, 0.f);
    push_sun(dirs, 60.f, 120.f);
    push_sun(dirs, -5.f, 240.f);
    const std::vector<float> weights = {0.5f, 2.f, 1.f};
    SunskySequence seq(parent, dirs, {2.5f, 6.f, 3.f}, weights);

    float dummy[4] = {0.f, 0.f, 1.f, 0.f};
    const std::vector<float> lam = variant == Variant::Spectral ? std::vector<float>{550.f} : std::vector<float>{};
    DirectionSample ds;
    ds.d = Vector3Out{dummy, dummy, dummy};
    ds.pdf = dummy;
    // before prepare_sampling: the message names the missing call
    const std::string a = error_of([&] { seq.sampling_info(); });
    std::printf("unprepared: %s\n", a.c_str());
    EXPECT(a.find("sunsky_sequence_prepare_sampling first") != std::string::npos);
    EXPECT(error_of([&] { seq.sample_direction(1, Point2{dummy, dummy}, ds, SpectrumOut{dummy, 1}, {}, lam); })
               .find("sunsky_sequence_prepare_sampling first") != std::string::npos);
    EXPECT(error_of([&] { seq.pdf_direction(1, DirectionSampleIn{Vector3{dummy, dummy, dummy}}, dummy); })
               .find("sunsky_sequence_prepare_sampling first") != std::string::npos);
    EXPECT(error_of([&] { seq.prepare_sampling(0, 16); }).find("sampling table size out of range") != std::string::npos);
    EXPECT(error_of([&] { seq.prepare_sampling(8, 2); }).find("sampling table size out of range") != std::string::npos);

    seq.prepare_sampling(8, 16);
    const sunsky_sequence_sampling_desc i = seq.sampling_info();
    EXPECT(i.n_z == 8 && i.n_phi == 16);
    EXPECT(i.w_sky > 0.f && i.w_sky < 1.f && i.sky_mass > 0.f && i.sun_mass > 0.f);
    EXPECT(std::fabs(i.w_sky - i.sky_mass / (i.sky_mass + i.sun_mass)) <= 1e-6f);
    const std::vector<float> f = seq.sampling_table(SUNSKY_SEQUENCE_TABLE_SKY);
    const std::vector<float> rows = seq.sampling_table(SUNSKY_SEQUENCE_TABLE_ROW_CDF);
    const std::vector<float> cells = seq.sampling_table(SUNSKY_SEQUENCE_TABLE_CELL_CDF);
    const std::vector<float> q = seq.sampling_table(SUNSKY_SEQUENCE_TABLE_Q);
    const std::vector<float> fcdf = seq.sampling_table(SUNSKY_SEQUENCE_TABLE_FRAME_CDF);
    const std::vector<float> B = seq.sampling_table(SUNSKY_SEQUENCE_TABLE_B);
    EXPECT(f.size() == 128 && cells.size() == 128 && rows.size() == 8 && q.size() == 3 && fcdf.size() == 3 && B.size() == 3);
    double S = 0.0;
    for (float v : f) {
        EXPECT(v >= 0.f);
        S += v;
    }
    EXPECT(std::fabs(S * 2.0 * 3.14159265358979 / 128.0 - i.sky_mass) <= 1e-5 * i.sky_mass);
    EXPECT(rows.back() == 1.f && fcdf.back() == 1.f && cells[15] == 1.f && cells.back() == 1.f);
    EXPECT(B[0] > 0.f && B[1] > 0.f && B[2] == 0.f && q[2] == 0.f);   // the third sun is below the horizon
    EXPECT(std::fabs(q[0] + q[1] - 1.f) <= 1e-6f);
    EXPECT(std::fabs(q[0] - weights[0] * B[0] / (weights[0] * B[0] + weights[1] * B[1])) <= 1e-6f);
    seq.prepare_sampling();   // the default 64 x 256 replaces the tables
    EXPECT(seq.sampling_info().n_z == 64 && seq.sampling_table(SUNSKY_SEQUENCE_TABLE_SKY).size() == 64 * 256);

    // prepared, but host-only: batch calls still need a device
    EXPECT(error_of([&] { seq.sample_direction(1, Point2{dummy, dummy}, ds, SpectrumOut{dummy, 1}, {}, lam); })
               .find("host-only sequence") != std::string::npos);
    EXPECT(error_of([&] { seq.pdf_direction(1, DirectionSampleIn{Vector3{dummy, dummy, dummy}}, dummy); })
               .find("host-only sequence") != std::string::npos);

    // a dark sequence (night only) has nothing to sample
    std::vector<float> night;
    push_sun(night, -5.f, 0.f);
    push_sun(night, -20.f, 90.f);
    SunskySequence dark(parent, night);
    const std::string d = error_of([&] { dark.prepare_sampling(8, 16); });
    std::printf("dark: %s\n", d.c_str());
    EXPECT(d.find("the sequence is dark") != std::string::npos);
}

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "host") != 0) {
        std::printf("usage: sequence_sampling_check host\n");
        return 2;
    }
    host_mode(Variant::RGB);
    host_mode(Variant::Spectral);
    if (failures) return 1;
    std::printf("sequence sampling host ok\n");
    return 0;
}
