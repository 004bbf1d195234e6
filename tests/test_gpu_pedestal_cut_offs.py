"""Wide cut-offs.  The pedestal pre-pass stages 2 x 16 runs of 2 cut_off + 3 slot sums in one
workgroup's LDS (pedestal.h): above 64 KiB its launches opt in, and cut-offs whose stage would
not fit a CU's 160 KiB are refused before any GPU work (LBL_MAX_PEDESTAL_CUT_OFF).  Without the
pedestal any cut-off is computed."""
import numpy as np
import pytest

from tests import golden_io
from tests.test_gpu_parity import assert_spectrum

pytestmark = pytest.mark.gpu

LIMIT = 305         # LBL_MAX_PEDESTAL_CUT_OFF (include/lbl_amd.h)
CUT_OFFS = (30, 31, 100, 114, 116, 130, 300, LIMIT, LIMIT + 1, 3000)
V0, VN = 1, 121


@pytest.fixture(scope="module")
def setup():
    from pylbl_amd import synthetic
    from pylbl_amd.engine import Engine
    engine = Engine(0)
    table = synthetic.line_table("O3", 1., 150., num_lines=500, seed=77, tips_range=(150, 400))
    yield engine, table, engine.load(table)
    engine.close()


def _ordinary_call_works(engine, molecule, oracle, table):
    k = engine.compute(molecule, 230., 5000., 4e-6, V0, VN, 4, remove_pedestal=True)[0]
    k_ref, _ = oracle.absorption_port(table, 230., 5000., 4e-6, V0, VN, 4, remove_pedestal=True)
    case = golden_io.Case("cut", 0, 0, 0, 0, V0, VN, 4, 25, True, None, 0)
    assert_spectrum(k, k_ref, case, "ordinary call after a refusal")


@pytest.mark.parametrize("cut_off", CUT_OFFS)
def test_wide_cut_offs(setup, oracle, cut_off):
    from pylbl_amd.errors import EngineError
    engine, table, molecule = setup
    try:
        for npv in (1, 16, 250):
            k_plain, _ = oracle.absorption_port(table, 230., 5000., 4e-6, V0, VN, npv,
                                                cut_off=cut_off)
            k_ref = None
            for farfield in (0, 1):
                for ped, scan in ((False, 1), (True, 1), (True, 0)):
                    engine.set_option("scan_chain", scan)
                    label = f"cut_off={cut_off} npv={npv} ped={ped} scan={scan} far={farfield}"
                    if ped and cut_off > LIMIT:
                        with pytest.raises(EngineError, match=f"LBL_MAX_PEDESTAL_CUT_OFF = {LIMIT}"):
                            engine.compute(molecule, 230., 5000., 4e-6, V0, VN, npv,
                                           cut_off=cut_off, remove_pedestal=True,
                                           farfield=bool(farfield))
                        _ordinary_call_works(engine, molecule, oracle, table)
                        continue
                    k = engine.compute(molecule, 230., 5000., 4e-6, V0, VN, npv, cut_off=cut_off,
                                       remove_pedestal=ped, farfield=bool(farfield))[0]
                    if ped and k_ref is None:
                        k_ref, _ = oracle.absorption_port(table, 230., 5000., 4e-6, V0, VN, npv,
                                                          cut_off=cut_off, remove_pedestal=True)
                    case = golden_io.Case("cut", 0, 0, 0, 0, V0, VN, npv, cut_off, ped, None, 0)
                    assert_spectrum(k, k_ref if ped else k_plain, case, label, k_plain)
    finally:
        engine.set_option("scan_chain", 1)


def test_refused_status_and_absorption_entry(setup, oracle, capfd):
    """The refusal is LBL_BAD_ARGUMENT at the C ABI; the reference-signature absorption() entry
    returns 1 and says why, and its next ordinary call still works."""
    from ctypes import byref, c_char_p, c_double, c_int, c_int64, c_void_p
    from pylbl_amd import engine as engine_module
    from pylbl_amd.database import write_database
    import os
    import tempfile
    engine, table, molecule = setup
    lib = engine_module.library()
    k = np.zeros(VN - V0)
    t, p, x = (np.asarray([v]) for v in (230., 5000., 4e-6))
    status = lib.lbl_compute(engine.handle, molecule, 1, t.ctypes.data, p.ctypes.data,
                             x.ctypes.data, V0, VN, 1, LIMIT + 1, 1, 0, 0, k.ctypes.data, 0,
                             byref(c_int64(0)))
    assert status == 2          # LBL_BAD_ARGUMENT
    assert f"LBL_MAX_PEDESTAL_CUT_OFF = {LIMIT}" in lib.lbl_last_error(engine.handle).decode()
    # (a function object of its own: other tests give the library's their own argument types)
    entry = lib["absorption"]
    entry.restype = c_int
    entry.argtypes = 3*[c_double] + 3*[c_int] + [c_void_p, c_char_p, c_char_p, c_int, c_int]
    with tempfile.TemporaryDirectory() as where:
        path = os.path.join(where, "lines.db")
        write_database(path, [table])
        for cut_off, expect in ((400, 1), (LIMIT + 1, 1), (LIMIT, 0), (25, 0)):
            k = np.full((VN - V0)*10, 3.)
            rc = entry(5000., 230., 4e-6, V0, VN, 10, k.ctypes.data, path.encode(),
                       b"O3", cut_off, 1)
            assert rc == expect, cut_off
            if expect:
                assert "LBL_MAX_PEDESTAL_CUT_OFF" in capfd.readouterr().err
                continue
            k_ref, _ = oracle.absorption_port(table, 230., 5000., 4e-6, V0, VN, 10,
                                              cut_off=cut_off, remove_pedestal=True)
            case = golden_io.Case("cut", 0, 0, 0, 0, V0, VN, 10, cut_off, True, None, 0)
            assert_spectrum(k, k_ref, case, f"absorption() cut_off={cut_off}")
