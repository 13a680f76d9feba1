// Drives the store pacer's rate controller (csrc/flat_pace.h) with a scripted sequence of launches -- plain C++17, no
// HIP -- and prints the state.  Built and run by tests/test_pace_rate_cpu.py.  Commands, in argv order:
//   start J GBS   the rate for a launch of J-float rows (a first or another J starts at GBS)
//   forget N      launches after which a ceiling is forgotten (default 10000)
//   slow N        N finished launches, each recorded at the CURRENT target, that took 1.2 x what the target explains
//   clean N       ... that took exactly what the target explains
//   stale N       N slow launches recorded at HALF the current target
//   reset         hgmm_pace_reset's part of the state
//   dump          one line: the state's fields as name=value
#include "flat_pace.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
    hgmm::PaceRate p;
    int forget = hgmm::PACE_FORGET_AFTER;
    const double bytes = 1e9;
    for (int i = 1; i < argc; ++i) {
        const char* cmd = argv[i];
        auto arg = [&]() { return ++i < argc ? std::atof(argv[i]) : 0.0; };
        auto launches = [&](double target_factor, double time_factor) {
            for (int n = (int)arg(); n > 0; --n) {
                const double recorded = p.target * target_factor;
                hgmm::pace_judge(p, recorded, bytes, time_factor * bytes / (recorded * 1e9) * 1e3, forget);
            }
        };
        if (!std::strcmp(cmd, "start")) { const int J = (int)arg(); hgmm::pace_rate_for(p, J, arg()); }
        else if (!std::strcmp(cmd, "forget")) forget = (int)arg();
        else if (!std::strcmp(cmd, "slow")) launches(1.0, 1.2);
        else if (!std::strcmp(cmd, "clean")) launches(1.0, 1.0);
        else if (!std::strcmp(cmd, "stale")) launches(0.5, 1.2);
        else if (!std::strcmp(cmd, "reset")) hgmm::pace_rate_reset(p);
        else if (!std::strcmp(cmd, "dump"))
            std::printf("target=%.17g J=%d strikes=%d steps_down=%d steps_up=%d ceiling=%.17g since_ceiling=%d "
                        "ceilings_forgotten=%d probe_base=%.17g clean=%d probe_after=%d probe_seen=%d\n",
                        p.target, p.J, p.strikes, p.steps_down, p.steps_up, p.ceiling, p.since_ceiling, p.ceilings_forgotten,
                        p.probe_base, p.clean, p.probe_after, p.probe_seen);
        else { std::fprintf(stderr, "unknown command %s\n", cmd); return 2; }
    }
    return 0;
}
