// fidget-hip: fidget-solver's solve (fidget-solver/src/lib.rs:191-289) for a batch of instances of one constraint system - the same
// tapes, each instance with its own parameter values - in one launch, the whole Levenberg-Marquardt loop on the device.
//
//   * one wave per workgroup; an instance owns a group of G lanes (solve_lm.hpp group_lanes: one gradient chunk of three free
//     variables per lane), so a wave carries 64 / G instances;
//   * the constraints' tapes are walked wave-uniformly by the step<> interpreter of the trait kernels (k_eval_grad / k_eval_f32):
//     GRAD for a Jacobian row, lane (g, j) evaluating chunk j of instance g (lib.rs:124-160), F32 for a trial error (lib.rs:163-190);
//     the register file is in LDS after the instances' work arrays, or in a global slab when it does not fit;
//   * an instance is a small state machine (Jacobian -> step -> trial -> ...), the wave loops until all of its instances are done;
//     the linear algebra of solve_lm.hpp runs with the rows of an instance spread over its lanes.  No host round trip per iteration.
#include "solve_lm.hpp"

struct SolveTape {
    uint64_t ops;     // device address of the constraint's ops (fhip_tape::d_ops)
    uint32_t len;     // ... their number
    uint32_t slots;   // where its slot map starts in SolveArgs::ints
};
// (few pointers: the kernel's scalar registers are spent on the interpreter)
struct SolveArgs {
    const SolveTape* tapes;      // per constraint
    const int32_t* ints;         // [n_params] parameter -> free index (-1: fixed), [n_free] free index -> parameter, then the slot
                                 // maps: tape input slot -> parameter (-1: no parameter, evaluates as 0)
    const float* values;         // [n_inst][n_params]
    float* res;                  // [n_inst][n_free] out, then [n_inst] err, iterations, exit reason
    GR* gregs;                   // global register files (nullptr: in LDS)
    uint32_t n_regs, n_constraints, n_params, n_free, n_inst, group, max_iterations;
};

enum : int { ST_JACOBIAN = 0, ST_STEP = 1, ST_TRIAL = 2, ST_DONE = 3 };

__global__ void __launch_bounds__(WAVE) k_solve(SolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t lane = threadIdx.x, G = a.group, per_wave = WAVE / G, n = a.n_free;
    const uint32_t g = lane / G, j = lane % G;
    const uint32_t inst = blockIdx.x * per_wave + g;
    const bool valid = inst < a.n_inst;
    const fhsolve::Layout L{n};
    const uint32_t stride = L.floats();
    float* S = (float*)smem + g * stride;
    float *cur = S + L.cur(), *delta = S + L.delta(), *row = S + L.row();
    char* rf = a.gregs ? (char*)(a.gregs + (size_t)blockIdx.x * a.n_regs * WAVE)
                       : smem + (((size_t)per_wave * stride * 4 + 15) & ~(size_t)15);
    const Regs<GR, WAVE> RG{(GR*)rf, (int)lane};
    const Regs<float, WAVE> RF{(float*)rf, (int)lane};
    const int32_t *free_of = a.ints, *param_of = a.ints + a.n_params;
    const float* vals = a.values + (size_t)(valid ? inst : 0) * a.n_params;
    const uint32_t n_chunks = fhsolve::chunk_count(n);
    const uint64_t group_mask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << (g * G);
    auto sync = [] { __syncthreads(); };
    auto any = [](bool b) { __syncthreads(); return __ballot(b) != 0; };   // (the workgroup is one wave: no LDS for the reduction)

    fhsolve::Lm st;
    fhsolve::lm_init(st);
    int state = valid ? ST_JACOBIAN : ST_DONE;
    if (valid)
        for (uint32_t k = j; k < n; k += G) cur[k] = vals[param_of[k]];
    sync();
    while (any(state != ST_DONE)) {
        if (any(state == ST_JACOBIAN)) {   // lib.rs:229-241: J and r at cur, accumulated into JᵀJ and Jᵀr row by row
            const bool act = state == ST_JACOBIAN, eval = act && j < n_chunks;
            if (act) fhsolve::accumulate_clear(S + L.jtj(), S + L.b(), n, j, G);
            bool all_zero = true;
            for (uint32_t i = 0; i < a.n_constraints; i++) {
                const AS4 SolveTape* T = (const AS4 SolveTape*)a.tapes + i;   // (wave-uniform: scalar loads)
                const ctape_t tape = (ctape_t)T->ops;
                const uint32_t len = T->len;
                const int32_t* sp = a.ints + T->slots;
                for (uint32_t k = 0; k < len; k++) {
                    step<GRAD, WAVE, true>(
                        tape[k], RG,
                        [&](uint32_t slot) {
                            const int32_t p = sp[slot];
                            if (p < 0) return gr1(0.0f);
                            const int32_t gi = free_of[p];
                            if (gi < 0) return gr1(vals[p]);
                            return gr(cur[gi], (uint32_t)gi == 3 * j ? 1.0f : 0.0f, (uint32_t)gi == 3 * j + 1 ? 1.0f : 0.0f,
                                      (uint32_t)gi == 3 * j + 2 ? 1.0f : 0.0f);
                        },
                        [&](uint32_t slot, GR v) {
                            if (!eval || slot != 0) return;
                            if (j == 0) S[L.resid()] = v.v;
                            if (3 * j < n) row[3 * j] = v.dx;
                            if (3 * j + 1 < n) row[3 * j + 1] = v.dy;
                            if (3 * j + 2 < n) row[3 * j + 2] = v.dz;
                        },
                        [](int) {});
                }
                sync();
                if (act) {
                    const float r = S[L.resid()];
                    all_zero = all_zero && r == 0.0f;
                    fhsolve::accumulate_row(S + L.jtj(), S + L.b(), row, r, n, j, G);
                }
                sync();
            }
            if (act) {
                if (all_zero) { st.exit = fhsolve::EXIT_ZERO_RESIDUAL; st.err_out = 0.0f; state = ST_DONE; }
                else state = ST_STEP;
            }
        }
        if (any(state == ST_STEP)) {       // lib.rs:243-250: the damped system's step
            const bool act = state == ST_STEP;
            fhsolve::solve_step(S, n, st.damping, act, j, G, sync, any);
            if (act) state = ST_TRIAL;
        }
        if (any(state == ST_TRIAL)) {      // lib.rs:252-258 (get_err: lib.rs:163-190), then lib.rs:262-285
            const bool act = state == ST_TRIAL, eval = act && j == 0;
            float err = 0.0f;
            for (uint32_t i = 0; i < a.n_constraints; i++) {
                const AS4 SolveTape* T = (const AS4 SolveTape*)a.tapes + i;   // (wave-uniform: scalar loads)
                const ctape_t tape = (ctape_t)T->ops;
                const uint32_t len = T->len;
                const int32_t* sp = a.ints + T->slots;
                for (uint32_t k = 0; k < len; k++) {
                    step<F32, WAVE, true>(
                        tape[k], RF,
                        [&](uint32_t slot) {
                            const int32_t p = sp[slot];
                            if (p < 0) return 0.0f;
                            const int32_t gi = free_of[p];
                            return gi < 0 ? vals[p] : cur[gi] - delta[gi];
                        },
                        [&](uint32_t slot, float v) { if (eval && slot == 0) err = err + v * v; },
                        [](int) {});
                }
            }
            if (eval) S[L.err()] = err;
            sync();
            bool take = false;
            if (act) {
                err = S[L.err()];
                take = fhsolve::lm_trial(st, err);
                if (!take) state = st.exit >= 0 ? ST_DONE : ST_STEP;
            }
            bool changed = false;
            if (take)
                for (uint32_t k = j; k < n; k += G) {
                    const float prev = cur[k], next = prev - delta[k];
                    changed |= prev != next;
                    cur[k] = next;
                }
            changed = (__ballot(changed) & group_mask) != 0;
            if (take) {
                fhsolve::lm_step_taken(st, err, changed, a.max_iterations);
                state = st.exit >= 0 ? ST_DONE : ST_JACOBIAN;
            }
            sync();
        }
    }
    if (valid) {
        float* r = a.res + (size_t)a.n_inst * n;
        for (uint32_t k = j; k < n; k += G) a.res[(size_t)inst * n + k] = cur[k];
        if (j == 0) {
            r[inst] = st.err_out;
            ((uint32_t*)r)[a.n_inst + inst] = st.iter;
            ((int32_t*)r)[2 * a.n_inst + inst] = st.exit;
        }
    }
}
