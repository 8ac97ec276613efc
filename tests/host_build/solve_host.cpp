// The constraint solver's host build: fidget_amd/csrc/solve_lm.hpp - the arithmetic k_solve runs - driven by the ORACLE's evaluators
// (orc_eval_grad_slice / orc_eval_point, handed in as function pointers), one instance after the other on each thread.  It is the
// CPU reference of fhip_solve: the oracle's evaluators equal the device's bit for bit, so the device solve equals this one bit for bit
// (tests/test_solver_host.py: the reference's solver tests; tests/test_solver_gpu.py: the device against this).  No GPU.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "solve_lm.hpp"

typedef int (*GradFn)(void* shape, const float* const* vars, uint32_t n_vars, uint32_t n, float* out);
typedef int (*PointFn)(void* shape, const float* vars, uint32_t n_vars, float* out, uint8_t* choices);

struct Problem {
    GradFn grad;
    PointFn point;
    void* const* shapes;
    const uint32_t *n_slots, *slot_off, *n_outputs;
    const int32_t* slot_param;   // per constraint from slot_off: input slot -> parameter, -1: none (evaluates as 0)
    uint32_t n_constraints, n_params, max_iterations;
    std::vector<int32_t> free_of, param_of;
};

static void solve_one(const Problem& P, const float* vals, float* out, float* err, uint32_t* iterations, int32_t* exit_reason) {
    const uint32_t n = (uint32_t)P.param_of.size(), nch = fhsolve::chunk_count(n);
    const fhsolve::Layout L{n};
    std::vector<float> S(L.floats());
    float *cur = S.data() + L.cur(), *delta = S.data() + L.delta(), *row = S.data() + L.row();
    for (uint32_t k = 0; k < n; k++) cur[k] = vals[P.param_of[k]];
    fhsolve::Lm st;
    fhsolve::lm_init(st);
    std::vector<std::vector<float>> gin;
    std::vector<const float*> gptr;
    std::vector<float> gout, pin, pout;
    auto nosync = [] {};
    auto any = [](bool b) { return b; };
    while (st.exit < 0) {
        // the Jacobian and the residuals at cur (lib.rs:124-160), accumulated into JᵀJ and Jᵀr row by row
        fhsolve::accumulate_clear(S.data() + L.jtj(), S.data() + L.b(), n, 0, 1);
        bool all_zero = true;
        for (uint32_t i = 0; i < P.n_constraints; i++) {
            const uint32_t ns = P.n_slots[i];
            gin.assign(ns ? ns : 1, std::vector<float>(4 * nch, 0.0f));
            gptr.resize(gin.size());
            for (uint32_t s = 0; s < ns; s++) {
                const int32_t p = P.slot_param[P.slot_off[i] + s];
                for (uint32_t j = 0; j < nch; j++) {
                    float* gv = &gin[s][4 * j];
                    if (p < 0) continue;
                    const int32_t gi = P.free_of[p];
                    if (gi < 0) { gv[0] = vals[p]; continue; }
                    gv[0] = cur[gi];
                    gv[1] = (uint32_t)gi == 3 * j ? 1.0f : 0.0f;
                    gv[2] = (uint32_t)gi == 3 * j + 1 ? 1.0f : 0.0f;
                    gv[3] = (uint32_t)gi == 3 * j + 2 ? 1.0f : 0.0f;
                }
            }
            for (size_t s = 0; s < gin.size(); s++) gptr[s] = gin[s].data();
            gout.assign((size_t)P.n_outputs[i] * nch * 4, 0.0f);
            P.grad(P.shapes[i], gptr.data(), ns, nch, gout.data());
            for (uint32_t j = 0; j < nch; j++)
                for (uint32_t c = 0; c < 3; c++)
                    if (3 * j + c < n) row[3 * j + c] = gout[4 * j + 1 + c];
            const float r = gout[0];
            all_zero = all_zero && r == 0.0f;
            fhsolve::accumulate_row(S.data() + L.jtj(), S.data() + L.b(), row, r, n, 0, 1);
        }
        if (all_zero) { st.exit = fhsolve::EXIT_ZERO_RESIDUAL; st.err_out = 0.0f; break; }
        // the damping loop (lib.rs:243-258)
        float e = 0.0f;
        for (;;) {
            fhsolve::solve_step(S.data(), n, st.damping, true, 0, 1, nosync, any);
            e = 0.0f;
            for (uint32_t i = 0; i < P.n_constraints; i++) {   // get_err (lib.rs:163-190)
                const uint32_t ns = P.n_slots[i];
                pin.assign(ns ? ns : 1, 0.0f);
                for (uint32_t s = 0; s < ns; s++) {
                    const int32_t p = P.slot_param[P.slot_off[i] + s];
                    if (p < 0) continue;
                    const int32_t gi = P.free_of[p];
                    pin[s] = gi < 0 ? vals[p] : cur[gi] - delta[gi];
                }
                pout.assign(P.n_outputs[i], 0.0f);
                P.point(P.shapes[i], pin.data(), ns, pout.data(), nullptr);
                e = e + pout[0] * pout[0];
            }
            if (fhsolve::lm_trial(st, e) || st.exit >= 0) break;
        }
        if (st.exit >= 0) break;
        bool changed = false;
        for (uint32_t k = 0; k < n; k++) {
            const float prev = cur[k], next = prev - delta[k];
            changed |= prev != next;
            cur[k] = next;
        }
        fhsolve::lm_step_taken(st, e, changed, P.max_iterations);
    }
    for (uint32_t k = 0; k < n; k++) out[k] = cur[k];
    *err = st.err_out;
    *iterations = st.iter;
    *exit_reason = st.exit;
}

// fhip_solve's arguments, with the slot maps made by the caller from the oracle's shapes.  Returns 0, or 6 (FHIP_ERR_UNSUPPORTED) for
// more than 64 free parameters.
extern "C" int fs_host_solve(void* grad, void* point, void* const* shapes, const uint32_t* n_slots, const uint32_t* n_outputs,
                             const int32_t* slot_param, uint32_t n_constraints, const uint8_t* param_free, uint32_t n_params,
                             const float* values, uint32_t n_instances, uint32_t max_iterations, uint32_t threads, float* out,
                             float* err, uint32_t* iterations, int32_t* exit_reason) {
    Problem P;
    P.grad = (GradFn)grad;
    P.point = (PointFn)point;
    P.shapes = shapes;
    P.n_slots = n_slots;
    P.n_outputs = n_outputs;
    P.slot_param = slot_param;
    P.n_constraints = n_constraints;
    P.n_params = n_params;
    P.max_iterations = max_iterations ? max_iterations : fhsolve::DEFAULT_MAX_ITERATIONS;
    P.free_of.assign(n_params, -1);
    for (uint32_t p = 0; p < n_params; p++)
        if (param_free[p]) { P.free_of[p] = (int32_t)P.param_of.size(); P.param_of.push_back((int32_t)p); }
    const uint32_t n = (uint32_t)P.param_of.size();
    if (n > fhsolve::MAX_FREE) return 6;
    std::vector<uint32_t> off(n_constraints);
    for (uint32_t i = 0, o = 0; i < n_constraints; i++) { off[i] = o; o += n_slots[i]; }
    P.slot_off = off.data();
    auto run = [&](uint32_t a, uint32_t b) {
        for (uint32_t s = a; s < b; s++)
            solve_one(P, values + (size_t)s * n_params, out + (size_t)s * n, err + s, iterations + s, exit_reason + s);
    };
    if (threads <= 1 || n_instances < 2) {
        run(0, n_instances);
        return 0;
    }
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++)
        pool.emplace_back(run, (uint32_t)((uint64_t)n_instances * t / threads), (uint32_t)((uint64_t)n_instances * (t + 1) / threads));
    for (auto& th : pool) th.join();
    return 0;
}
