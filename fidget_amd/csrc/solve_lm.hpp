// fidget-hip: the arithmetic of fidget-solver's Levenberg-Marquardt loop (fidget-solver/src/lib.rs:191-289) as per-instance steps,
// shared by the device solver (solve.hip: k_solve, one lane group per instance) and its host build (tests/host_build/solve_host.cpp,
// driven by the oracle's evaluators).  Written with + - * /, sqrtf and fabsf only and built with -ffp-contract=off on both sides, so
// the two compute the same bits.
//
// Every element of the work arrays has one owner and a fixed order of operations: a loop over elements takes (k0, kstep) - the host
// passes (0, 1), lane j of a group of G lanes passes (j, G) - and `sync` separates the reads of a phase from its writes (a barrier on
// the device, nothing on the host).  An instance's result therefore depends on its own inputs only: not on G, the batch size or its
// place in the batch.
//
// Deliberate differences from the reference (SOLVER.md):
//   * free variables are numbered in the caller's parameter order (the reference's HashMap order varies from run to run);
//   * the outer loop stops after `max_iterations` accepted steps and the damping loop after MAX_RETRIES rejected trials in a row,
//     each with its own exit reason (the reference loops without bound);
//   * the step is the pseudo-inverse of the damped system A = JᵀJ + damping · diag(JᵀJ) from its eigen-decomposition by cyclic
//     Jacobi (A is symmetric positive semi-definite: sigma_k = |lambda_k|), not nalgebra's Golub-Kahan SVD; singular values
//     <= f32::EPSILON count as zero, as in SVD::solve(b, eps).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define FS_HD __attribute__((always_inline)) inline
#endif

namespace fhsolve {

// exit reasons (include/fidget_hip.h FHIP_SOLVE_*)
enum : int32_t {
    EXIT_ZERO_RESIDUAL = 0,   // every residual was exactly 0 (lib.rs:234-236)
    EXIT_NO_CHANGE = 1,       // the accepted step changed no component (lib.rs:275)
    EXIT_ZERO_ERROR = 2,      // err == 0 (lib.rs:276)
    EXIT_ZERO_DAMPING = 3,    // damping == 0 (lib.rs:277)
    EXIT_STALLED = 4,         // the last four errors are equal (lib.rs:278)
    EXIT_MAX_ITERATIONS = 5,  // max_iterations steps accepted (not in the reference)
    EXIT_MAX_RETRIES = 6,     // MAX_RETRIES trials in a row rejected (not in the reference)
};
constexpr uint32_t MAX_FREE = 64;
constexpr uint32_t DEFAULT_MAX_ITERATIONS = 1000;
constexpr uint32_t MAX_RETRIES = 128;
constexpr uint32_t JACOBI_SWEEPS = 32;
constexpr float F32_EPSILON = 1.1920929e-7f;   // f32::EPSILON

// lanes per instance: the smallest power of two >= ceil(n_free / 3) (one gradient chunk of three free variables per lane), <= 64
FS_HD uint32_t group_lanes(uint32_t n_free) {
    const uint32_t chunks = (n_free + 2) / 3;
    uint32_t g = 1;
    while (g < chunks && g < 64) g *= 2;
    return g;
}
// gradient chunks of one Jacobian row: at least one, whose value is the residual (all parameters fixed included)
FS_HD uint32_t chunk_count(uint32_t n_free) { return n_free ? (n_free + 2) / 3 : 1; }

// An instance's work arrays, in floats from its base: JᵀJ, A (damped, then diagonalised), V (eigenvectors), b = Jᵀr, cur, delta,
// w (Vᵀb / lambda), the current Jacobian row, then two scalars (the residual of the current row, the trial error)
struct Layout {
    uint32_t n;
    FS_HD uint32_t jtj() const { return 0; }
    FS_HD uint32_t a() const { return n * n; }
    FS_HD uint32_t v() const { return 2 * n * n; }
    FS_HD uint32_t b() const { return 3 * n * n; }
    FS_HD uint32_t cur() const { return 3 * n * n + n; }
    FS_HD uint32_t delta() const { return 3 * n * n + 2 * n; }
    FS_HD uint32_t w() const { return 3 * n * n + 3 * n; }
    FS_HD uint32_t row() const { return 3 * n * n + 4 * n; }
    FS_HD uint32_t resid() const { return 3 * n * n + 5 * n; }
    FS_HD uint32_t err() const { return 3 * n * n + 5 * n + 1; }
    FS_HD uint32_t floats() const { return 3 * n * n + 5 * n + 2; }
};

// The loop's scalars (lib.rs:218-221), one copy per lane of the instance's group
struct Lm {
    float damping, prev_err, err_out;
    float e0, e1, e2, e3;   // err_buf's four entries, oldest first (a shift, not a ring indexed by i % 4: a runtime-indexed array of a
                            // lane lives in scratch; "all equal" does not depend on the order)
    uint32_t iter, retries;
    int32_t exit;           // < 0 while running
};
FS_HD void lm_init(Lm& s) {
    s.damping = 1.0f;
    s.prev_err = INFINITY;
    s.err_out = INFINITY;   // the error at the returned point: +inf until a step is accepted
    s.e0 = s.e1 = s.e2 = s.e3 = 0.0f;
    s.iter = 0;
    s.retries = 0;
    s.exit = -1;
}
// the damping loop's test of a trial error (lib.rs:247-257); true: accept the step.  A NaN error is accepted, as there.
FS_HD bool lm_trial(Lm& s, float err) {
    if (err > s.prev_err) {
        s.damping *= 1.5f;
        if (++s.retries >= MAX_RETRIES) s.exit = EXIT_MAX_RETRIES;
        return false;
    }
    s.damping /= 3.0f;
    s.retries = 0;
    return true;
}
// after cur -= delta (lib.rs:262-285): the error buffer and the exits, in the reference's order
FS_HD void lm_step_taken(Lm& s, float err, bool changed, uint32_t max_iterations) {
    s.e0 = s.e1; s.e1 = s.e2; s.e2 = s.e3; s.e3 = err;
    s.iter++;
    s.err_out = err;
    if (!changed) s.exit = EXIT_NO_CHANGE;
    else if (err == 0.0f) s.exit = EXIT_ZERO_ERROR;
    else if (s.damping == 0.0f) s.exit = EXIT_ZERO_DAMPING;
    else if (s.e1 == s.e0 && s.e2 == s.e0 && s.e3 == s.e0) s.exit = EXIT_STALLED;
    else {
        s.prev_err = err;
        if (s.iter >= max_iterations) s.exit = EXIT_MAX_ITERATIONS;
    }
}

// JᵀJ and Jᵀr start at zero for a new Jacobian
FS_HD void accumulate_clear(float* jtj, float* b, uint32_t n, uint32_t k0, uint32_t kstep) {
    for (uint32_t e = k0; e < n * n + n; e += kstep) {
        if (e < n * n) jtj[e] = 0.0f;
        else b[e - n * n] = 0.0f;
    }
}
// ... and add one row of J (constraint order, ascending): jtj[a][c] += J_a J_c, b[a] += J_a r
FS_HD void accumulate_row(float* jtj, float* b, const float* row, float r, uint32_t n, uint32_t k0, uint32_t kstep) {
    for (uint32_t e = k0; e < n * n + n; e += kstep) {
        if (e < n * n) jtj[e] = jtj[e] + row[e / n] * row[e % n];
        else b[e - n * n] = b[e - n * n] + row[e - n * n] * r;
    }
}
// A = JᵀJ + damping · diag(JᵀJ) (lib.rs:244-245: a_kk + damping * a_kk), V = identity
FS_HD void damped_system(const float* jtj, float* A, float* V, float damping, uint32_t n, uint32_t k0, uint32_t kstep) {
    for (uint32_t e = k0; e < n * n; e += kstep) {
        const bool diag = e / n == e % n;
        A[e] = diag ? jtj[e] + damping * jtj[e] : jtj[e];
        V[e] = diag ? 1.0f : 0.0f;
    }
}
// The rotation that zeroes A[p][q] (cyclic Jacobi, classic form); false: the entry is negligible next to both diagonal entries
// (or 0), and the pair is left alone.  A sweep that rotates nothing ends the iteration.
FS_HD bool jacobi_rotation(float app, float aqq, float apq, float& t, float& s, float& tau) {
    const float g = 100.0f * fabsf(apq);
    if (fabsf(app) + g == fabsf(app) && fabsf(aqq) + g == fabsf(aqq)) return false;
    const float h = aqq - app;
    if (fabsf(h) + g == fabsf(h)) {
        t = apq / h;
    } else {
        const float theta = 0.5f * h / apq;
        t = 1.0f / (fabsf(theta) + sqrtf(1.0f + theta * theta));
        if (theta < 0.0f) t = -t;
    }
    const float c = 1.0f / sqrtf(1.0f + t * t);
    s = t * c;
    tau = s / (1.0f + c);
    return true;
}
// One pair (p, q) of a sweep over the symmetric n x n matrix A and its eigenvectors V (both row major): every lane reads the
// rotation's three entries, then updates its rows k.  Returns whether it rotated.
template <class Sync>
FS_HD bool jacobi_pair(float* A, float* V, uint32_t n, uint32_t p, uint32_t q, bool active, uint32_t k0, uint32_t kstep, Sync sync) {
    const float app = A[p * n + p], aqq = A[q * n + q], apq = A[p * n + q];
    float t = 0.0f, s = 0.0f, tau = 0.0f;
    const bool rot = active && jacobi_rotation(app, aqq, apq, t, s, tau);
    sync();
    if (rot) {
        for (uint32_t k = k0; k < n; k += kstep) {
            if (k != p && k != q) {
                const float akp = A[k * n + p], akq = A[k * n + q];
                const float nkp = akp - s * (akq + tau * akp), nkq = akq + s * (akp - tau * akq);
                A[k * n + p] = nkp; A[p * n + k] = nkp;
                A[k * n + q] = nkq; A[q * n + k] = nkq;
            }
            const float vkp = V[k * n + p], vkq = V[k * n + q];
            V[k * n + p] = vkp - s * (vkq + tau * vkp);
            V[k * n + q] = vkq + s * (vkp - tau * vkq);
        }
        if (k0 == 0) {
            A[p * n + p] = app - t * apq;
            A[q * n + q] = aqq + t * apq;
            A[p * n + q] = 0.0f;
            A[q * n + p] = 0.0f;
        }
    }
    sync();
    return rot;
}
// delta = V · diag(1/lambda_k, or 0 where |lambda_k| <= f32::EPSILON) · Vᵀ b, in two phases: w = the scaled Vᵀb ...
FS_HD void pinv_weights(const float* A, const float* V, const float* b, float* w, uint32_t n, uint32_t k0, uint32_t kstep) {
    for (uint32_t m = k0; m < n; m += kstep) {
        const float lam = A[m * n + m];
        float acc = 0.0f;
        for (uint32_t j = 0; j < n; j++) acc = acc + V[j * n + m] * b[j];
        w[m] = fabsf(lam) > F32_EPSILON ? acc / lam : 0.0f;
    }
}
// ... then delta = V w
FS_HD void pinv_step(const float* V, const float* w, float* d, uint32_t n, uint32_t k0, uint32_t kstep) {
    for (uint32_t k = k0; k < n; k += kstep) {
        float acc = 0.0f;
        for (uint32_t m = 0; m < n; m++) acc = acc + V[k * n + m] * w[m];
        d[k] = acc;
    }
}
// The step of the damped system whose JᵀJ and Jᵀr are in `base`: A, V, the Jacobi sweeps, w and delta.  `any` reduces a flag over
// everything that runs in lockstep (the wave on the device), so that a sweep loop ends together for all; an instance that has
// converged rotates nothing in the sweeps that follow.
template <class Sync, class Any>
FS_HD void solve_step(float* base, uint32_t n, float damping, bool active, uint32_t k0, uint32_t kstep, Sync sync, Any any) {
    const Layout L{n};
    float *A = base + L.a(), *V = base + L.v();
    if (active) damped_system(base + L.jtj(), A, V, damping, n, k0, kstep);
    sync();
    bool busy = active;
    for (uint32_t sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
        if (!any(busy)) break;
        bool rotated = false;
        for (uint32_t p = 0; p + 1 < n; p++)
            for (uint32_t q = p + 1; q < n; q++) rotated |= jacobi_pair(A, V, n, p, q, busy, k0, kstep, sync);
        busy = busy && rotated;
    }
    if (active) pinv_weights(A, V, base + L.b(), base + L.w(), n, k0, kstep);
    sync();
    if (active) pinv_step(V, base + L.w(), base + L.delta(), n, k0, kstep);
    sync();
}

}  // namespace fhsolve
