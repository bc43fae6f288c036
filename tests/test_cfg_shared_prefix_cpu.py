"""The switch of the guidance pair's shared prefix, host side, no GPU: the entry point of include/gligen_amd_sampler.h is declared,
exported and bound, rejects what is no switch position, and the row-policy report's tail shows the position."""
import ctypes
import os
import re

from helpers import ROOT


def test_sampler_entry_point_is_declared_exported_and_bound():
    from gligen_amd import _lib
    from gligen_amd.build import build_native
    build_native()
    header = open(os.path.join(ROOT, "include", "gligen_amd_sampler.h")).read()
    declared = set(re.findall(r"\b(gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SAMPLER_SYMBOLS) == {"gl_set_cfg_shared_prefix"}
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert all(hasattr(lib, n) for n in declared)
    assert not declared & set(_lib.SYMBOLS)
    _lib.load()


def test_switch_positions_and_report_tail():
    from gligen_amd import _lib
    lib = _lib.load()

    def tail():
        buf = ctypes.create_string_buffer(4096)
        assert lib.gl_ff_rows_policy_report(buf, 4096) == 0
        m = re.search(r";cfg_shared_prefix=(\d) evals=(\d+) rows_at_prefix=(\d+) rows_periodic=(\d+)$", buf.value.decode())
        assert m, buf.value
        return int(m.group(1))

    try:
        assert tail() == 1                                   # the default
        assert lib.gl_set_cfg_shared_prefix(0) == 0 and tail() == 0
        assert lib.gl_set_cfg_shared_prefix(2) != 0 and lib.gl_set_cfg_shared_prefix(-1) != 0 and tail() == 0
        assert b"shared prefix" in lib.gl_last_error()
    finally:
        assert lib.gl_set_cfg_shared_prefix(1) == 0 and tail() == 1
