// The store pacer's rate controller: plain C++, no HIP type and no HIP header, so that its rules run on any host
// (tests/pace_rate_main.cpp feeds it scripted launches).  What measures a launch -- event pairs and the workgroups'
// wall-clock stamps -- is the measurement ring of hgmm_ctx.h (PaceRing), driven from flat_kernels.hip.
#pragma once
#include <algorithm>

namespace hgmm {

// Offered store rate of the paced N x J writers (materialising E-step, estimate_log_prob), GB/s.  The knee of the write
// path sat at 6.8 - 7.0 TB/s on every box of round 4, but it is a property of the memory system's state (refresh rate
// with temperature, the stacks of the particular chip), and past it the kernel does not degrade gracefully -- it drops
// to ~5.3 TB/s; the knee is soft besides: at 6700 one launch in three already ran 3 - 18 % long in bursts, at 6600 the
// 150 launches of a bench run stayed within 488 - 506 us of their 487 (profiles/r04).  So the rate starts at 6600 and is
// CONTROLLED: a paced launch that runs more than 6 % longer than its
// target explains counts as a strike, three strikes in a row lower the target by 2 % (never below PACE_FLOOR_GBS).  The
// evidence comes from event pairs around the last few launches that are queried -- never waited for -- at the next
// launch, so the stream is not disturbed.  Launches that are not store-bound by construction (the row-maximum loop,
// small tables) neither adapt nor are they judged.  HGMM_ESTEP_TARGET_GBS=<n> fixes the rate (0: un-paced), HGMM_ESTEP_ADAPT=0
// keeps the initial one.
constexpr int ESTEP_TARGET_GBS = 6600;
constexpr double PACE_FLOOR_GBS = 5800.0;
constexpr double PACE_STRIKE_RATIO = 1.06;
constexpr double PACE_STEP = 0.98;
constexpr double PACE_MIN_BYTES = 256.0 * 1024 * 1024;
// ... and upwards, carefully: the knee sat at 7.0 TB/s on one box and at 7.6 on another (profiles/r04/paced_fill_lease*.log).
// After PACE_PROBE_AFTER clean launches in a row the rate is raised by 2 % on probation: three clean launches keep it, the
// first long one takes it back, remembers the rate as a ceiling and doubles the wait before the next probe.
// ... and a ceiling is a statement about the memory system's state WHEN it was learnt (another stream writing at the same
// time, a hot chip), not for life: after PACE_FORGET_AFTER clean launches below it (HGMM_PACE_FORGET=<n>) it is forgotten and
// the probes start over with their first waiting time.  hgmm_pace_reset() forgets everything at once.
constexpr int PACE_FORGET_AFTER = 10000;
constexpr int PACE_PROBE_AFTER = 24, PACE_PROBE_AFTER_MAX = 4096;
constexpr double PACE_PROBE_STEP = 1.02;
constexpr double PACE_CEILING_GBS = 7600.0;

struct PaceRate {
    double target = 0.0;               // GB/s offered by the next paced launch; 0: not initialised
    int strikes = 0;                   // consecutive launches that ran longer than their target explains
    int J = 0;                         // the row length the state belongs to (another J starts over)
    int steps_down = 0;                // how often the target was lowered (reported by hgmm_pace_info)
    int steps_up = 0;                  // probes upwards that held
    // probing upwards: after `probe_after` clean launches in a row the next ones are offered 2 % more; three clean ones
    // make that the new target, a single long one ends the probe, caps the rate below it and doubles `probe_after`
    double ceiling = 1e30;             // a rate that was seen to congest: not probed again until it is forgotten
    int since_ceiling = 0;             // clean launches since the ceiling was learnt (forgotten after `forget_after`)
    int ceilings_forgotten = 0;
    double probe_base = 0.0;           // > 0: a probe is running, this is the rate to fall back to
    int clean = 0, probe_after = 0, probe_seen = 0;
};

// the rate the next paced launch of J-float rows offers: the state's own, or `start_gbs` afresh for a first or another J
inline double pace_rate_for(PaceRate& p, int J, double start_gbs) {
    if (p.target <= 0.0 || p.J != J) {
        p.target = start_gbs;
        p.strikes = p.clean = p.probe_seen = 0;
        p.probe_after = PACE_PROBE_AFTER;
        p.probe_base = 0.0;
        p.ceiling = 1e30;
        p.since_ceiling = 0;
        p.J = J;
    }
    return p.target;
}

// one finished launch: offered `recorded_target` GB/s of `bytes` bytes, it took `ms`.  A launch recorded under another
// target than the current one says nothing about the current one.
inline void pace_judge(PaceRate& p, double recorded_target, double bytes, double ms, int forget_after) {
    if (recorded_target != p.target) return;
    const double ideal_ms = bytes / (recorded_target * 1e9) * 1e3;
    const bool slow = ms > PACE_STRIKE_RATIO * ideal_ms;
    if (p.probe_base > 0.0) {
        // a probe is running: ONE long launch ends it (the memory system has said no), three clean ones accept it
        if (slow) {
            p.ceiling = p.target;
            p.since_ceiling = 0;
            p.target = p.probe_base;
            p.probe_base = 0.0;
            p.probe_after = std::min(PACE_PROBE_AFTER_MAX, 2 * p.probe_after);
            p.clean = 0;
            p.strikes = 0;
        } else if (++p.probe_seen >= 3) {
            p.probe_base = 0.0;
            p.steps_up++;
            p.clean = 0;
        }
    } else if (slow) {
        p.clean = 0;
        if (++p.strikes >= 3) {
            p.ceiling = std::min(p.ceiling, p.target);
            p.since_ceiling = 0;
            p.target = std::max(PACE_FLOOR_GBS, p.target * PACE_STEP);
            p.strikes = 0;
            p.steps_down++;
        }
    } else {
        p.strikes = 0;
        if (p.ceiling < 1e29 && ++p.since_ceiling >= forget_after) {
            p.ceiling = 1e30;                       // what congested then need not congest now: probe afresh
            p.since_ceiling = 0;
            p.probe_after = PACE_PROBE_AFTER;
            p.ceilings_forgotten++;
        }
        const double up = p.target * PACE_PROBE_STEP;
        if (++p.clean >= p.probe_after && up < p.ceiling * 0.995 && up <= PACE_CEILING_GBS) {
            p.probe_base = p.target;
            p.target = up;
            p.probe_seen = 0;
        }
    }
}

// hgmm_pace_reset: the next paced launch starts over (pace_rate_for), the counters with it
inline void pace_rate_reset(PaceRate& p) {
    p.target = 0.0;
    p.steps_down = p.steps_up = p.ceilings_forgotten = 0;
}

}  // namespace hgmm
