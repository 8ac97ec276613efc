"""The constraint solver (fidget::solver): `Free`, `Fixed`, `solve`, `solve_batch`."""
import ctypes as C

import numpy as np

from ._abi import STATUS, _p, lib
from .context import default_context


# ---- constraint solver (fidget::solver, fidget-solver/src/lib.rs) ---------------------------------------------------------
class Free(float):
    """Parameter::Free(start) (fidget-solver/src/lib.rs:11-17): a variable the solver moves, from this start"""


class Fixed(float):
    """Parameter::Fixed(value): a variable held at this value"""


SOLVE_EXITS = {0: "zero_residual", 1: "no_change", 2: "zero_error", 3: "zero_damping", 4: "stalled", 5: "max_iterations",
               6: "max_retries"}       # include/fidget_hip.h FHIP_SOLVE_*
SOLVE_MAX_FREE = 64


def solve_key(key):
    """'x' | 'y' | 'z' | int (a Var::V index, as Context.var) -> (axis, index) of fhip_solve"""
    if isinstance(key, str):
        return "xyz".index(key.lower()), 0
    return 3, int(key)


def solve_batch(constraints, keys, free_mask, values, max_iterations=0, hip=None):
    """fhip_solve: every row of `values` ([n_instances][n_params]: the start of a free parameter, the value of a fixed one) is one
    solve of the same constraints (a list of Shape; residual = output 0).  keys: per parameter 'x' | 'y' | 'z' | int; free_mask:
    per parameter, true = free.  Returns (out [n_instances][n_free] - the free parameters in parameter order -, err, iterations,
    exit_reason - SOLVE_EXITS)."""
    keys = list(keys)
    free = np.ascontiguousarray(np.asarray(free_mask, dtype=bool).reshape(len(keys)), dtype=np.uint8)
    vals = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1, len(keys)))
    n_inst, n_free = vals.shape[0], int(free.sum())
    ax = np.array([solve_key(k)[0] for k in keys], dtype=np.int32)
    ix = np.array([solve_key(k)[1] for k in keys], dtype=np.uint64)
    hip = hip or (constraints[0].hip if constraints else default_context())
    tapes = (C.c_void_p * max(len(constraints), 1))(*[s._h.value for s in constraints])
    out = np.zeros((n_inst, n_free), dtype=np.float32)
    err = np.zeros(n_inst, dtype=np.float32)
    its = np.zeros(n_inst, dtype=np.uint32)
    ex = np.zeros(n_inst, dtype=np.int32)
    st = lib().fhip_solve(hip._h, tapes, len(constraints), _p(ax), _p(ix), _p(free), len(keys), _p(vals), n_inst,
                          int(max_iterations), _p(out), _p(err), _p(its), _p(ex))
    if st in (1, 5, 6):
        raise ValueError(f"{STATUS[st]}: {lib().fhip_last_error(hip._h).decode()}")
    hip.check(st)
    return out, err, its, ex


def solve(constraints, params, max_iterations=0, hip=None):
    """fidget::solver::solve (fidget-solver/src/lib.rs:191): params maps 'x' | 'y' | 'z' | int to Free(start) or Fixed(value);
    returns {key: value} for the free variables"""
    keys = list(params)
    for k in keys:
        if not isinstance(params[k], (Free, Fixed)):
            raise TypeError(f"parameter {k!r}: Free(v) or Fixed(v), not {params[k]!r}")
    free = [isinstance(params[k], Free) for k in keys]
    out = solve_batch(constraints, keys, free, [[float(params[k]) for k in keys]], max_iterations, hip)[0][0]
    return {k: float(v) for k, v in zip([k for k, f in zip(keys, free) if f], out)}
