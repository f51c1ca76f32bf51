"""The device SQP's C ABI and Python face, as far as they can be held without a GPU: the two entry points are declared and
exported, the ctypes mirrors of smpc_sqp_opts / smpc_sqp_state match the header, and generate_guess(on_device=True) refuses a
solver that has no device SQP."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT


def test_sqp_entry_points_declared_and_exported():
    from safe_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(ROOT, 'include', 'smpc.h')).read()
    declared = set(re.findall(r'^int\s+(smpc_[a-z_]+)\s*\(', hdr, re.M))
    L = C.CDLL(_lib.LIB_PATH)
    for name in ('smpc_merit_terms', 'smpc_sqp_batch'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name


def test_sqp_structs_match_the_header(tmp_path):
    """sizeof / offsetof of smpc_sqp_opts and smpc_sqp_state compiled from the header with gcc against the ctypes mirrors"""
    from safe_mpc_amd import _lib
    O, S = _lib.SqpOpts, _lib.SqpState
    of = [n for n, _ in O._fields_]
    sf = [n for n, _ in S._fields_]
    fmt = ' '.join(['%zu'] * (2 + len(of) + len(sf)))
    args = ', '.join(['sizeof(smpc_sqp_opts)', 'sizeof(smpc_sqp_state)'] + [f'offsetof(smpc_sqp_opts, {n})' for n in of] +
                     [f'offsetof(smpc_sqp_state, {n})' for n in sf])
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smpc.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    v = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert v == [C.sizeof(O), C.sizeof(S)] + [getattr(O, n).offset for n in of] + [getattr(S, n).offset for n in sf]
    # the defaults are those of generate_guess
    o = O()
    assert (o.max_iter, o.tol, o.armijo, o.alpha_reduction, o.alpha_min, o.mu0, o.mu_max) == (1, 1e-6, 1e-4, 0.7, 0.05, 10.0, 1e8)
    assert [n for n, _ in S.FIELDS] == sf


def test_generate_guess_on_device_needs_a_device_sqp():
    """the oracle-backed controller has no device SQP: a clear ValueError, not a silent host loop"""
    from fake_solver import make_double_controller
    from safe_mpc_amd import closed_loop as cl
    from safe_mpc_amd.parser import Parameters
    par = Parameters({}, 'z1')
    par.nq, par.n_dof_safe_set, par.net_size, par.N, par.nlp_max_iter = 6, 6, [12, 256, 1], 20, 200
    with pytest.raises(ValueError, match='device SQP'):
        cl.generate_guess(par, 'htwa', 48, make_controller=lambda n, b: make_double_controller(n, par, b), on_device=True)
