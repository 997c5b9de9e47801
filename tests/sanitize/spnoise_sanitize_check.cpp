// The sequential two-port noise solve of engine/ac_port_noise.hpp under ASan + UBSan: a stand-alone program with
// exactly sized heap buffers, so that any index past a work plane, a solution, Y, Cy or the generator table aborts.
// Built and run by tests/test_spnoise_sanitize.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ac_port_noise.hpp"

namespace {

// a small deterministic generator (no <random>: the values only have to be finite and the same everywhere)
struct Lcg {
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 - 0.5; }
};

int run(int n, int P, int S, bool singular, Lcg& rng)
{
    const int ld = n + P;
    std::vector<double> G(n * n), C(n * n), psd(S), ar(n * ld), ai(n * ld), xr(P * n), xi(P * n);
    std::vector<double> yr(P * P), yi(P * P), cr(P * P), ci(P * P);
    std::vector<int32_t> pe(P), sa(S), sb(S);
    for (int e = 0; e < n * n; ++e) { G[e] = rng.next(); C[e] = rng.next(); }
    for (int i = 0; i < n; ++i) G[i * n + (n - 1 - i)] += 4.0 * n;             // pivots off the diagonal: rows are exchanged
    if (singular)
        for (int i = 0; i < n; ++i) { G[(n / 2) * n + i] = 0.0; C[(n / 2) * n + i] = 0.0; }
    const int ports[4] = {0, n - 1, n / 2, (n - 1) / 3};
    for (int i = 0; i < P; ++i) pe[i] = ports[i];
    for (int s = 0; s < S; ++s) {
        sa[s] = s % (n + 1) - 1;                                              // -1 (ground) .. n - 1
        sb[s] = (3 * s + 1) % (n + 1) - 1;
        psd[s] = s == 2 ? 0.0 : 1.6e-20 * (rng.next() + 0.6);
    }
    unsigned flags = 0u;
    double sum = 0.0;
    const double omega[3] = {1.0, 0.0, 2.5};
    for (double w : omega) {
        csim::TwoPortNoise tp{};
        flags |= csim::ac_spnoise_solve(n, G.data(), C.data(), w, P, pe.data(), S, sa.data(), sb.data(), psd.data(),
                                        4.0 * 1.380649e-23 * 290.0, 1.0 / 50.0, 1e-15, ld, ar.data(), ai.data(), xr.data(),
                                        xi.data(), yr.data(), yi.data(), cr.data(), ci.data(), P == 2 ? &tp : nullptr);
        for (int e = 0; e < P * P; ++e) sum += yr[e] + yi[e] + cr[e] + ci[e];
        sum += tp.rn;
    }
    std::printf("n %d P %d S %d flags %u checksum %.17g\n", n, P, S, flags, sum);
    return singular == (flags != 0u) ? 0 : 1;
}

} // namespace

int main()
{
    Lcg rng{20250822ull};
    int bad = 0;
    for (int n : {2, 9, 33, 63})
        for (int P = 1; P <= 4; ++P)
            for (int S : {0, 1, 5, 65}) {
                bad += run(n, P, S, false, rng);
                if (S == 5) bad += run(n, P, S, true, rng);
            }
    return bad ? 1 : 0;
}
