"""The refusals of the time loops and eigensolvers on the LOD space, word for word: for every single bad argument that
the test_lod_*_abi.py files list for a call, the return code and the full error text.  The argument checks of these
calls are written once per scheme (slod_lod_time.hip, slod_lod_wave.hip, slod_lod_eig.hip); this table was recorded from
the library before they were merged, so that a call keeps its own wording: which calls answer a NULL handle with a bare
code and which leave a text, "n_rhs" or "n_members" in the leading-dimension message, the factor looked at last.

  python tests/test_lod_loops_messages.py     prints the table as the library of this tree answers (EXPECTED below)

No GPU is needed: every case is refused before any device work.  A text of None stands for a bare code: the call leaves
the error text as it found it."""
import ctypes as C
import os
import sys

import pytest

FAKE = 1 << 20   # never dereferenced: the argument checks reject the call first
NAN, INF = float("nan"), float("inf")
K, STEPS, M = 3, 4, 6   # columns or members, time steps, eigensolver block


def _calls(h, rows):
    """name -> (good arguments but for a NULL factor, ((position, bad value), ...), fix or None).  (1, None) on a call
    that takes a factor changes nothing: with every other argument in order the NULL factor is what is refused."""
    its, res = (C.c_int * 8)(), (C.c_double * 8)()
    out = (C.c_double * K)()
    kin, pot = (C.c_double * ((STEPS + 1) * K))(), (C.c_double * ((STEPS + 1) * K))()
    lam, rsd = (C.c_double * (64 * K))(), (C.c_double * (64 * K))()
    status = (C.c_int * K)()

    def wide(at_block, at_ld, scale):       # so that only n_block is wrong
        def fix(a, at, bad):
            if at == at_block and bad > M:
                a[at_ld] = scale * bad
        return fix

    return {
        "slod_lod_theta_steps": (
            [h, FAKE, FAKE, FAKE, 0.01, 1.0, STEPS, K, FAKE, K, FAKE, K, 0, 1e-12, 10, its, res],
            ((0, None), (1, None), (2, None), (3, None), (8, None), (4, 0.0), (4, -0.01), (4, NAN), (5, -0.1), (5, 1.1),
             (5, NAN), (6, 0), (6, -1), (7, 0), (7, -1), (9, K - 1), (11, K - 1), (14, -1)), None),
        "slod_lod_theta_steps_direct": (
            [h, None, FAKE, FAKE, 0.01, 0.5, STEPS, K, FAKE, K, FAKE, K, 0],
            ((0, None), (2, None), (3, None), (8, None), (4, 0.0), (4, -0.01), (4, NAN), (5, -0.01), (5, 1.01), (5, NAN),
             (6, 0), (6, -1), (7, 0), (7, -1), (9, K - 1), (11, K - 1), (1, None)), None),
        "slod_lod_theta_steps_ensemble_direct": (
            [h, None, FAKE, K, FAKE, 0.01, 1.0, 1, K, FAKE, K, FAKE, K, 0],
            ((0, None), (2, None), (4, None), (9, None), (5, 0.0), (5, -0.01), (5, NAN), (6, -0.1), (6, 1.1), (6, NAN),
             (7, 0), (8, 0), (8, -1), (8, 65536), (3, K - 1), (10, K - 1), (12, K - 1), (1, None)), None),
        "slod_lod_inner_multi": (
            [h, FAKE, FAKE, FAKE, K, FAKE, K, K, out, None],
            ((0, None), (1, None), (2, None), (3, None), (5, None), (8, None), (7, 0), (7, -1), (4, K - 1), (6, K - 1)),
            None),
        "slod_lod_inner_ensemble": (
            [h, FAKE, K, FAKE, FAKE, K, FAKE, K, K, out, None],
            ((0, None), (1, None), (3, None), (4, None), (6, None), (9, None), (8, 0), (8, -1), (8, 65536), (2, K - 1),
             (5, K - 1), (7, K - 1)), None),
        "slod_lod_newmark_accel": (
            [h, FAKE, FAKE, FAKE, 0.1, 0.01, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 1e-12, 10, its, res],
            ((0, None), (1, None), (2, None), (3, None), (7, None), (9, None), (13, None), (4, -0.1), (4, NAN), (5, -0.1),
             (5, NAN), (6, 0), (6, -1), (8, K - 1), (10, K - 1), (12, K - 1), (14, K - 1), (16, -1)), None),
        "slod_lod_newmark_accel_direct": (
            [h, None, FAKE, FAKE, FAKE, 0.1, 0.01, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K],
            ((0, None), (2, None), (3, None), (4, None), (8, None), (10, None), (14, None), (5, -0.1), (5, NAN), (6, -0.1),
             (6, NAN), (7, 0), (7, -1), (9, K - 1), (11, K - 1), (13, K - 1), (15, K - 1), (1, None)), None),
        "slod_lod_newmark_accel_ensemble_direct": (
            [h, None, FAKE, K, FAKE, K, FAKE, 0.0, 0.0, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K],
            ((0, None), (2, None), (4, None), (6, None), (10, None), (12, None), (16, None), (9, 0), (9, -1), (9, 65536),
             (3, K - 1), (5, K - 1), (11, K - 1), (13, K - 1), (15, K - 1), (17, K - 1), (7, -0.1), (7, NAN), (8, -1e-3),
             (8, NAN), (1, None)), None),
        "slod_lod_newmark_steps": (
            [h, FAKE, FAKE, FAKE, 0.01, 0.25, 0.5, 0.1, 0.01, STEPS, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 0, 1e-12, 10, its,
             res, kin, pot],
            ((0, None), (1, None), (2, None), (3, None), (11, None), (13, None), (15, None), (4, 0.0), (4, -0.01), (4, NAN),
             (5, -0.01), (5, 0.51), (5, NAN), (6, -0.01), (6, 1.01), (6, NAN), (7, -0.1), (7, NAN), (8, -0.1), (8, NAN),
             (9, 0), (9, -1), (10, 0), (10, -1), (12, K - 1), (14, K - 1), (16, K - 1), (18, K - 1), (21, -1), (24, None),
             (25, None)), None),
        "slod_lod_newmark_steps_direct": (
            [h, None, FAKE, FAKE, FAKE, 0.01, 0.25, 0.5, 0.1, 0.01, STEPS, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 0, kin, pot],
            ((0, None), (2, None), (3, None), (4, None), (12, None), (14, None), (16, None), (5, 0.0), (5, -0.01), (5, NAN),
             (6, -0.01), (6, 0.51), (6, NAN), (7, -0.01), (7, 1.01), (7, NAN), (8, -0.1), (8, NAN), (9, -0.1), (9, NAN),
             (10, 0), (10, -1), (11, 0), (11, -1), (13, K - 1), (15, K - 1), (17, K - 1), (19, K - 1), (21, None), (22, None),
             (1, None)), None),
        "slod_lod_newmark_steps_ensemble_direct": (
            [h, None, FAKE, K, FAKE, K, FAKE, 0.01, 0.25, 0.5, 0.0, 0.0, 1, K, FAKE, K, FAKE, K, FAKE, K, FAKE, K, 0, kin, pot],
            ((0, None), (2, None), (4, None), (6, None), (14, None), (16, None), (18, None), (7, 0.0), (7, -0.01), (7, NAN),
             (8, 0.6), (8, -0.1), (8, NAN), (9, -0.1), (9, 1.1), (9, NAN), (10, -0.1), (10, NAN), (11, -1e-3), (11, NAN),
             (12, 0), (12, -1), (13, 0), (13, -1), (13, 65536), (3, K - 1), (5, K - 1), (15, K - 1), (17, K - 1), (19, K - 1),
             (21, K - 1), (23, None), (24, None), (1, None)), None),
        "slod_lod_eigs": (
            [h, FAKE, FAKE, FAKE, 2, M, 0, FAKE, M, 1e-10, 5, 1e-12, 100, lam, rsd, its],
            ((0, None), (1, None), (2, None), (3, None), (7, None), (13, None), (14, None), (4, 0), (4, -1), (4, M + 1),
             (5, 65), (5, rows + 1), (8, M - 1), (6, 2), (6, -1), (9, 0.0), (9, -1e-10), (9, NAN), (11, 0.0), (11, -1e-12),
             (11, NAN), (10, 0), (10, -1), (12, -1)), wide(5, 8, 1)),
        "slod_lod_eigs_direct": (
            [h, None, FAKE, FAKE, FAKE, 2, M, 0, FAKE, M, 1e-10, 5, lam, rsd],
            ((0, None), (2, None), (3, None), (4, None), (8, None), (12, None), (13, None), (5, 0), (5, -1), (5, M + 1),
             (6, 65), (6, rows + 1), (9, M - 1), (7, 2), (7, -1), (10, 0.0), (10, -1e-10), (10, NAN), (11, 0), (11, -1),
             (1, None)), wide(6, 9, 1)),
        "slod_lod_eigs_ensemble_direct": (
            [h, None, FAKE, K, FAKE, K + 1, FAKE, K, 2, M, 0, FAKE, K * M, 1e-10, 5, lam, rsd, status],
            ((0, None), (2, None), (4, None), (6, None), (11, None), (15, None), (16, None), (17, None), (8, 0), (8, -1),
             (8, M + 1), (9, 65), (9, rows + 1), (10, 2), (10, -1), (13, 0.0), (13, -1e-10), (13, NAN), (14, 0), (14, -1),
             (7, 0), (7, -1), (7, 65536), (3, K - 1), (5, K - 1), (12, K * M - 1), (12, M), (1, None)), wide(9, 12, K)),
        "slod_lod_eigs_shift_direct": (
            [h, None, 3.5, FAKE, FAKE, FAKE, 2, M, 0, FAKE, M, 1e-10, 5, lam, rsd],
            ((0, None), (3, None), (4, None), (5, None), (9, None), (13, None), (14, None), (2, NAN), (2, INF), (2, -INF),
             (6, 0), (6, -1), (6, M + 1), (7, 65), (7, rows + 1), (10, M - 1), (8, 2), (8, -1), (11, 0.0), (11, -1e-10),
             (11, NAN), (12, 0), (12, -1), (1, None)), wide(7, 10, 1)),
        "slod_lod_eigs_shift_ensemble_direct": (
            [h, None, -2.0, FAKE, K, FAKE, K + 1, FAKE, K, 2, M, 0, FAKE, K * M, 1e-10, 5, lam, rsd, status],
            ((0, None), (3, None), (5, None), (7, None), (12, None), (16, None), (17, None), (18, None), (2, NAN), (2, INF),
             (9, 0), (9, -1), (9, M + 1), (10, 65), (10, rows + 1), (11, 2), (11, -1), (14, 0.0), (14, -1e-10), (14, NAN),
             (15, 0), (15, -1), (8, 0), (8, -1), (8, 65536), (4, K - 1), (6, K - 1), (13, K * M - 1), (13, M), (1, None)),
            wide(10, 13, K)),
    }


def _observe(g, name):
    """[(return code, error text or None)] of the cases of `name`, in order.  Before every case the handle's text and the
    thread's are set to known ones by two refusals of calls outside this table; a call that leaves the text it found
    answered with a bare code."""
    lib = g.lib
    ok, cases, fix = _calls(g.h, g.num_patches * g.spacedim)[name]
    fn, seen = getattr(lib, name), []
    for at, bad in cases:
        assert lib.slod_lod_apply_multi(g.h, FAKE, FAKE, FAKE, 1, 0, 2 * FAKE, 1, None) == -1
        assert lib.slod_lod_factor_solve_ensemble(None, 0, K, FAKE, K, 1, FAKE, K, None) == -1
        before = [lib.slod_last_error(g.h).decode(), lib.slod_last_error(None).decode()]
        assert "slod_lod_apply_multi" in before[0] and "slod_lod_factor_solve_ensemble" in before[1]
        a = list(ok)
        a[at] = bad
        if fix:
            fix(a, at, bad)
        rc = fn(*a)
        after = [lib.slod_last_error(g.h).decode(), lib.slod_last_error(None).decode()]
        mine = 1 if at == 0 else 0                          # a NULL handle: the thread's text
        assert after[1 - mine] == before[1 - mine], (name, at, bad, "wrote the other text")
        seen.append((rc, None if after[mine] == before[mine] else after[mine]))
    return seen


# as recorded from the library before the argument checks were merged
EXPECTED = {
    'slod_lod_eigs': [
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, 'slod_lod_eigs: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs: leading dimension below n_block'),
        (-1, 'slod_lod_eigs: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs: tol or inner_rel_tol is not positive'),
        (-1, 'slod_lod_eigs: tol or inner_rel_tol is not positive'),
        (-1, 'slod_lod_eigs: tol or inner_rel_tol is not positive'),
        (-1, 'slod_lod_eigs: tol or inner_rel_tol is not positive'),
        (-1, 'slod_lod_eigs: tol or inner_rel_tol is not positive'),
        (-1, 'slod_lod_eigs: tol or inner_rel_tol is not positive'),
        (-1, 'slod_lod_eigs: max_outer < 1 or inner_max_iterations < 0'),
        (-1, 'slod_lod_eigs: max_outer < 1 or inner_max_iterations < 0'),
        (-1, 'slod_lod_eigs: max_outer < 1 or inner_max_iterations < 0'),
    ],
    'slod_lod_eigs_direct': [
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_direct: leading dimension below n_block'),
        (-1, 'slod_lod_eigs_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_direct: NULL factor'),
    ],
    'slod_lod_eigs_ensemble_direct': [
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL member_status'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_ensemble_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_ensemble_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_ensemble_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_ensemble_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_ensemble_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_ensemble_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_ensemble_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_eigs_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_eigs_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_eigs_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_eigs_ensemble_direct: leading dimension below n_members * n_block'),
        (-1, 'slod_lod_eigs_ensemble_direct: leading dimension below n_members * n_block'),
        (-1, 'slod_lod_eigs_ensemble_direct: NULL factor'),
    ],
    'slod_lod_eigs_shift_direct': [
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_direct: sigma is NaN or infinite'),
        (-1, 'slod_lod_eigs_shift_direct: sigma is NaN or infinite'),
        (-1, 'slod_lod_eigs_shift_direct: sigma is NaN or infinite'),
        (-1, 'slod_lod_eigs_shift_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_shift_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_shift_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_shift_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_shift_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_shift_direct: leading dimension below n_block'),
        (-1, 'slod_lod_eigs_shift_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_shift_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_shift_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_shift_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_shift_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_shift_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_shift_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_shift_direct: NULL factor'),
    ],
    'slod_lod_eigs_shift_ensemble_direct': [
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL handle, matrix, d_cols, d_x, eigenvalues or residuals'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL member_status'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: sigma is NaN or infinite'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: sigma is NaN or infinite'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_eig < 1 or n_block < n_eig'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_block above 64 or above the number of rows'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: start is neither 0 nor 1'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: tol is not positive'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: max_outer < 1'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: leading dimension below n_members * n_block'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: leading dimension below n_members * n_block'),
        (-1, 'slod_lod_eigs_shift_ensemble_direct: NULL factor'),
    ],
    'slod_lod_inner_ensemble': [
        (-1, 'slod_lod_inner_ensemble: NULL handle or array'),
        (-1, 'slod_lod_inner_ensemble: NULL handle or array'),
        (-1, 'slod_lod_inner_ensemble: NULL handle or array'),
        (-1, 'slod_lod_inner_ensemble: NULL handle or array'),
        (-1, 'slod_lod_inner_ensemble: NULL handle or array'),
        (-1, 'slod_lod_inner_ensemble: NULL handle or array'),
        (-1, 'slod_lod_inner_ensemble: n_members < 1 or > 65535'),
        (-1, 'slod_lod_inner_ensemble: n_members < 1 or > 65535'),
        (-1, 'slod_lod_inner_ensemble: n_members < 1 or > 65535'),
        (-1, 'slod_lod_inner_ensemble: leading dimension below n_members'),
        (-1, 'slod_lod_inner_ensemble: leading dimension below n_members'),
        (-1, 'slod_lod_inner_ensemble: leading dimension below n_members'),
    ],
    'slod_lod_inner_multi': [
        (-1, None),
        (-1, 'slod_lod_inner_multi: NULL array'),
        (-1, 'slod_lod_inner_multi: NULL array'),
        (-1, 'slod_lod_inner_multi: NULL array'),
        (-1, 'slod_lod_inner_multi: NULL array'),
        (-1, 'slod_lod_inner_multi: NULL array'),
        (-1, 'slod_lod_inner_multi: n_rhs < 1'),
        (-1, 'slod_lod_inner_multi: n_rhs < 1'),
        (-1, 'slod_lod_inner_multi: leading dimension below n_rhs'),
        (-1, 'slod_lod_inner_multi: leading dimension below n_rhs'),
    ],
    'slod_lod_newmark_accel': [
        (-1, None),
        (-1, 'slod_lod_newmark_accel: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel: n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_accel: n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_accel: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel: n_rhs < 1 or max_iterations < 0'),
    ],
    'slod_lod_newmark_accel_direct': [
        (-1, None),
        (-1, 'slod_lod_newmark_accel_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_direct: n_rhs < 1'),
        (-1, 'slod_lod_newmark_accel_direct: n_rhs < 1'),
        (-1, 'slod_lod_newmark_accel_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_accel_direct: NULL factor'),
    ],
    'slod_lod_newmark_accel_ensemble_direct': [
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_accel_ensemble_direct: NULL factor'),
    ],
    'slod_lod_newmark_steps': [
        (-1, None),
        (-1, 'slod_lod_newmark_steps: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_steps: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_newmark_steps: kinetic and potential come together or not at all'),
        (-1, 'slod_lod_newmark_steps: kinetic and potential come together or not at all'),
    ],
    'slod_lod_newmark_steps_direct': [
        (-1, None),
        (-1, 'slod_lod_newmark_steps_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_direct: NULL matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_newmark_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_newmark_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_newmark_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_newmark_steps_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_newmark_steps_direct: kinetic and potential come together or not at all'),
        (-1, 'slod_lod_newmark_steps_direct: kinetic and potential come together or not at all'),
        (-1, 'slod_lod_newmark_steps_direct: NULL factor'),
    ],
    'slod_lod_newmark_steps_ensemble_direct': [
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL handle, matrix, d_cols or state'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: dt <= 0, beta outside [0, 1/2] or gamma outside [0, 1]'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: negative or NaN damping coefficient'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: n_steps < 1'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: n_steps < 1'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: n_members < 1 or > 65535'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: kinetic and potential come together or not at all'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: kinetic and potential come together or not at all'),
        (-1, 'slod_lod_newmark_steps_ensemble_direct: NULL factor'),
    ],
    'slod_lod_theta_steps': [
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, None),
        (-1, 'slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_theta_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_theta_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_theta_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
        (-1, 'slod_lod_theta_steps: leading dimension below n_rhs'),
        (-1, 'slod_lod_theta_steps: leading dimension below n_rhs'),
        (-1, 'slod_lod_theta_steps: n_steps < 1, n_rhs < 1 or max_iterations < 0'),
    ],
    'slod_lod_theta_steps_direct': [
        (-1, None),
        (-1, 'slod_lod_theta_steps_direct: NULL matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_direct: NULL matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_direct: NULL matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_theta_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_theta_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_theta_steps_direct: n_steps < 1 or n_rhs < 1'),
        (-1, 'slod_lod_theta_steps_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_theta_steps_direct: leading dimension below n_rhs'),
        (-1, 'slod_lod_theta_steps_direct: NULL factor'),
    ],
    'slod_lod_theta_steps_ensemble_direct': [
        (-1, 'slod_lod_theta_steps_ensemble_direct: NULL handle, matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: NULL handle, matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: NULL handle, matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: NULL handle, matrix, d_cols or d_u'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: dt <= 0 or theta outside [0, 1]'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: n_steps < 1, n_members < 1 or > 65535'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: n_steps < 1, n_members < 1 or > 65535'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: n_steps < 1, n_members < 1 or > 65535'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: n_steps < 1, n_members < 1 or > 65535'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: leading dimension below n_members'),
        (-1, 'slod_lod_theta_steps_ensemble_direct: NULL factor'),
    ],
}


NAMES = sorted(EXPECTED)


def test_the_table_covers_every_call():
    assert NAMES == sorted(_calls(None, 16))
    assert len(NAMES) == 16


@pytest.mark.parametrize("spacedim", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_lod_loops_refusals_word_for_word(name, spacedim):
    import slod_amd
    g = slod_amd.Slod(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
    _, cases, _ = _calls(g.h, g.num_patches * spacedim)[name]
    seen, want = _observe(g, name), EXPECTED[name]
    assert len(seen) == len(want) == len(cases)
    for (at, bad), got, exp in zip(cases, seen, want):
        assert got == exp, (name, at, bad)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-slod_amd"))
    import slod_amd
    tables = []
    for spacedim in (1, 2):
        g = slod_amd.Slod(nref=2, n_sub=2, oversampling=1, spacedim=spacedim, n_problems=3)
        tables.append({name: _observe(g, name) for name in sorted(_calls(None, 16))})
    assert tables[0] == tables[1], "the texts depend on spacedim"
    print("EXPECTED = {")
    for name, seen in tables[0].items():
        print("    %r: [" % name)
        for rc, text in seen:
            print("        (%d, %r)," % (rc, text))
        print("    ],")
    print("}")
