"""What Session.decay must leave in a resident session (include/poismf_hip.h section 2e), in numpy alone: no GPU code.  Used by
tests/test_session_scale_cpu.py (which checks it by hand-worked cases) and tests/test_gpu_session_decay.py."""
import numpy as np
import scipy.sparse as sp

from tests import helpers as H


def expected(X, gamma, su, si, floor, prec):
    """(E, n_gone, any_non_finite): the stored cells of the SciPy matrix X (distinct, or integer-valued so that summing duplicates is
    exact) after nv = ((x * gamma) * su[row]) * si[col] -- three separate multiplications in the session's dtype, each rounded once, su /
    si None: ones -- with a cell kept if and only if nv > floor; E is CSR with sorted indices, n_gone the cells that left, any_non_finite
    whether some nv is not finite (the call then refuses and E is not what the session holds)."""
    dt = H.dtype_of(prec)
    Xs = sp.csr_matrix(X).astype(dt)
    Xs.sum_duplicates()
    coo = Xs.tocoo()
    row, col, x = coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(dt)
    su = np.ones(X.shape[0], dt) if su is None else np.asarray(su).astype(dt)
    si = np.ones(X.shape[1], dt) if si is None else np.asarray(si).astype(dt)
    assert su.shape == (X.shape[0],) and si.shape == (X.shape[1],)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a = x * dt(gamma)
        b = a * su[row]
        nv = b * si[col]
    assert a.dtype == b.dtype == nv.dtype == dt
    keep = nv > dt(floor)
    E = sp.csr_matrix((nv[keep], (row[keep], col[keep])), shape=X.shape, dtype=dt)
    E.sort_indices()
    assert E.nnz == int(keep.sum())
    return E, int((~keep).sum()), bool(not np.isfinite(nv).all())
