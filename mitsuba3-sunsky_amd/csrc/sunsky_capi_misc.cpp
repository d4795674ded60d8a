// sunsky_capi_misc.cpp -- the entry points of the C ABI (include/sunsky_amd.h) that take no
// handle: version, last error, sun coordinates, array files, the Hosek sun radiance, paths.
#include "sunsky_dataset.h"
#include "sunsky_launch.h"

using namespace sunsky;
using namespace sunsky::capi;

namespace sunsky {
double hosek_solar_radiance(const std::string& datasets, double turbidity, double wavelength, double elevation,
                            double gamma);
}

extern "C" {

int sunsky_abi_version(void) { return SUNSKY_AMD_ABI_VERSION; }
const char* sunsky_last_error(void) { return last_error().c_str(); }

int sunsky_sun_coordinates(int year, int month, int day, float hour, float minute, float second, float latitude,
                           float longitude, float timezone, float out[3]) {
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    DateTime t;
    t.year = year; t.month = month; t.day = day; t.hour = hour; t.minute = minute; t.second = second;
    Location l;
    l.latitude = latitude; l.longitude = longitude; l.timezone = timezone;
    compute_sun_coordinates(t, l, out);
    return SUNSKY_OK;
}

int sunsky_array_from_file(const char* path, int file_dtype, double* out, size_t cap, size_t* count, uint64_t* shape,
                           int* ndims) {
    if (!path || !count) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    Table t;
    std::string err;
    if (!read_array_file(path, file_dtype, &t, &err))
        return fail(err.find("does not exist") != std::string::npos ? SUNSKY_ERROR_FILE : SUNSKY_ERROR_FORMAT, err);
    *count = t.size();
    if (out) std::memcpy(out, t.data.data(), sizeof(double) * std::min(cap, t.size()));
    if (ndims) *ndims = (int)t.shape.size();
    if (shape)
        for (size_t i = 0; i < t.shape.size() && i < 16; ++i) shape[i] = t.shape[i];
    return SUNSKY_OK;
}

int sunsky_array_to_file(const char* path, const float* data, size_t count, const uint64_t* shape, int ndims) {
    if (!path || (!data && count)) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    std::vector<size_t> sh;
    for (int i = 0; i < ndims; ++i) sh.push_back((size_t)shape[i]);
    std::string err;
    if (!write_array_file(path, data, count, sh.empty() ? nullptr : sh.data(), (int)sh.size(), &err))
        return fail(SUNSKY_ERROR_FILE, err);
    return SUNSKY_OK;
}

const char* plugin_name(void) { return "sunsky"; }
const char* plugin_descr(void) { return "Sun and Sky dome background emitter (MI355X)"; }

int sunsky_hosek_sun_rad(const char* dataset_path, double turbidity, double wavelength, double elevation,
                         double gamma, double* out) {
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    return guarded([&] {
        std::string ds = dataset_path && *dataset_path ? std::string(dataset_path) : default_pack_path();
        *out = hosek_solar_radiance(ds, turbidity, wavelength, elevation, gamma);
    });
}

int sunsky_default_dataset_path(char* buf, size_t cap) {
    if (!buf || !cap) return fail(SUNSKY_ERROR_INVALID_VALUE, "null buffer");
    std::snprintf(buf, cap, "%s", default_pack_path().c_str());
    return SUNSKY_OK;
}

}  // extern "C"
