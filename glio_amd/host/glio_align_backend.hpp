// glio_align_backend.hpp -- the GNSS frame estimate on the C-ABI of include/glio_align.h.  C-ABI only, C++14, no HIP headers.
//
//   glio::GnssAlignment   the device object (glio_align_*): yaw_enu_local and anc_ecef from a local trajectory and the DD pseudorange factors along it.  It
//                         replaces what the reference reads from the yaml (yaw_enu_local, anc_ecef) and from the ground-truth heading
//                         (Estimator.cpp:1434-1448); the frame goes into glio_set_gnss / glio_batch_set_small_factors unchanged.
// The Python twin is glio_amd/align.py.
#ifndef GLIO_ALIGN_BACKEND_HPP_
#define GLIO_ALIGN_BACKEND_HPP_
#include <stdexcept>
#include <string>
#include <vector>

#include "glio_align.h"

namespace glio {

class GnssAlignment {
public:
    struct Result { glio_gnss_frame frame; glio_align_info info; bool delivered() const { return info.status != GLIO_ALIGN_UNOBSERVABLE; } };

    GnssAlignment(int max_factors, int max_positions, int device = 0) { check(glio_align_create(device, max_factors, max_positions, &h_), "glio_align_create"); }
    ~GnssAlignment() { glio_align_destroy(h_); }
    GnssAlignment(const GnssAlignment&) = delete;
    GnssAlignment& operator=(const GnssAlignment&) = delete;
    glio_align* handle() const { return h_; }

    static glio_align_opts defaultOpts() { glio_align_opts o; glio_align_opts_default(&o); return o; }
    void setOpts(const glio_align_opts& o) { check(glio_align_set_opts(h_, &o), "glio_align_set_opts"); }
    void setFactors(const std::vector<glio_dd_psr>& dd) { check(glio_align_set_factors(h_, (int)dd.size(), dd.data()), "glio_align_set_factors"); }
    // position k at base[k * stride_doubles]: a [n][7] pose table is passed as it lies
    void setPositions(const double* base, int n, int stride_doubles = 3) { check(glio_align_set_positions(h_, n, base, stride_doubles), "glio_align_set_positions"); }
    // throws on a refusal; an UNOBSERVABLE result returns the start frame (delivered() == false)
    Result solve(const glio_gnss_frame& start) {
        Result r;
        check(glio_align_solve(h_, &start, &r.frame, &r.info), "glio_align_solve");
        return r;
    }
    double cost(const glio_gnss_frame& frame, double threshold, int32_t* n_downweighted = nullptr) {
        double c = 0;
        check(glio_align_cost(h_, &frame, threshold, &c, n_downweighted), "glio_align_cost");
        return c;
    }
    // the reduced costs of the last solve's hypotheses
    std::vector<double> readCoarse() {
        int32_t n = 0;
        check(glio_align_read_coarse(h_, nullptr, 0, &n), "glio_align_read_coarse");
        std::vector<double> out((size_t)n);
        check(glio_align_read_coarse(h_, out.data(), n, nullptr), "glio_align_read_coarse");
        return out;
    }
    float lastDeviceMs() { float ms = 0; check(glio_align_last_device_ms(h_, &ms), "glio_align_last_device_ms"); return ms; }

private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_align* h_ = nullptr;
};

}  // namespace glio
#endif  // GLIO_ALIGN_BACKEND_HPP_
