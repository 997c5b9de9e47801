// pz_sanitize_check -- engine/pz.hpp under AddressSanitizer and UBSan: pz_poles() on three embedded systems with exactly
// sized heap buffers (tests/test_pz_sanitize.py builds and runs this once).  Prints one line per system.
//
//   1. the series RLC of tests/golden/ac_rlc_series.sp (n = 5: a conjugate pair, three eigenvalues the cut drops)
//   2. an RC ladder of n = 63 (the largest size: every work plane at its bound, real poles only)
//   3. a singular G + sigma0 C (n = 4: the failure path writes NaN slots)
#include <cmath>
#include <cstdio>
#include <vector>

#include "pz.hpp"

namespace {

int run(const char* name, int n, const std::vector<double>& G, const std::vector<double>& C, double sigma0, double fmax,
        unsigned wantFlags, int wantPoles)
{
    const int ld = n | 1;
    // the planes hold n rows of ld doubles and nothing more; the last row needs only n of them
    std::vector<double> a0((size_t)(n - 1) * ld + n), m((size_t)(n - 1) * ld + n), wr(n), wi(n), poles(2 * (size_t)n);
    int np = -1, nr = -1;
    double mx = 0.0;
    const unsigned fl = csim::pz_poles(n, G.data(), C.data(), sigma0, csim::pz_wmax(fmax), 1e-15, ld, a0.data(), m.data(),
                                       wr.data(), wi.data(), poles.data(), &np, &nr, &mx);
    std::printf("%s: flags 0x%x, %d poles, %d in the right half plane, max_re %.17g\n", name, fl, np, nr, mx);
    if (fl != wantFlags || np != wantPoles) return 1;
    for (int k = 0; k < n; ++k)
        if ((k < np) != (poles[2 * k] == poles[2 * k])) return 1;       // NaN exactly beyond n_poles
    return 0;
}

} // namespace

int main()
{
    int bad = 0;
    {
        const int n = 5;
        std::vector<double> G(n * n, 0.0), C(n * n, 0.0);
        const double g = 0.02, gmin = 1e-6;
        G[0 * n + 0] = g + gmin; G[0 * n + 1] = -g; G[0 * n + 3] = 1.0;
        G[1 * n + 0] = -g; G[1 * n + 1] = g + gmin; G[1 * n + 4] = 1.0;
        G[2 * n + 2] = gmin; G[2 * n + 4] = -1.0;
        G[3 * n + 0] = 1.0;
        G[4 * n + 1] = 1.0; G[4 * n + 2] = -1.0;
        C[2 * n + 2] = 1e-9;
        C[4 * n + 4] = -1e-6;
        bad += run("series RLC", n, G, C, 0.0, 1e12, 0u, 2);
    }
    {
        const int n = 63;
        std::vector<double> G(n * n, 0.0), C(n * n, 0.0);
        for (int i = 0; i < n; ++i) {
            G[i * n + i] = (i == n - 1 ? 1e-3 : 2e-3) + 1e-6;
            if (i > 0) G[i * n + i - 1] = -1e-3;
            if (i < n - 1) G[i * n + i + 1] = -1e-3;
            C[i * n + i] = 1e-12 * (1 + i % 3);
        }
        bad += run("RC ladder", n, G, C, -1e3, 1e13, 0u, 63);
    }
    {
        const int n = 4;
        std::vector<double> G(n * n, 0.0), C(n * n, 0.0);
        G[0] = 1.0; G[1] = -1.0; G[n] = -1.0; G[n + 1] = 1.0; G[2 * n + 2] = 1.0;
        C[0] = 1e-9; C[2 * n + 2] = 1e-9;
        bad += run("singular", n, G, C, 0.0, 1e12, CSIM_ST_PZ_SINGULAR, 0);
    }
    return bad ? 1 : 0;
}
