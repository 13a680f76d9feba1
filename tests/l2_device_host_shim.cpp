// csrc/l2_device.h built for the HOST (tests/test_l2_device_host_cpu.py): the serial part of the device L2 solve behind a
// C interface, so that the very text the step kernel runs is held to tests/_l2_solve_model.py on a CPU.
#include <cstring>

#include "l2_device.h"

using namespace hgmm;

extern "C" int l2h_state_size() { return (int)sizeof(L2SolveState); }

// the state as hgmm_l2_solve uploads it: zeros, the start point, the limits
extern "C" void l2h_init(L2SolveState* s, const double* x, int max_iter, double gtol) {
    std::memset(s, 0, sizeof *s);
    std::memcpy(s->x, x, sizeof s->x);
    s->max_iter = max_iter;
    s->gtol = gtol;
}

// what l2_solve_pose writes into a hypothesis' slot
extern "C" void l2h_pose(const double* theta, double* rot) {
    L2Quat q;
    l2_quat_terms(theta, false, q);
    std::memcpy(rot, q.rot, sizeof q.rot);
}

extern "C" void l2h_step(L2SolveState* s, const double* out13) { l2_solve_step(*s, out13); }

// ints: nit, nfev, status, left
extern "C" void l2h_get(const L2SolveState* s, double* x, double* f, double* g, int* ints, double* xt) {
    std::memcpy(x, s->x, sizeof s->x);
    *f = s->f;
    std::memcpy(g, s->g, sizeof s->g);
    ints[0] = s->nit; ints[1] = s->nfev; ints[2] = s->status; ints[3] = s->left;
    std::memcpy(xt, s->xt, sizeof s->xt);
}
