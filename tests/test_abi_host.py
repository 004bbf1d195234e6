"""CPU-only: pylbl_amd/abi.py against include/lbl_amd.h, whole.  Every function the header
declares has one prototype in abi.PROTOTYPES, in the header's order, with the header's argument
count, argument types and result type; struct lbl_band is BandDescriptor; every #define is
mirrored, or listed here with the place that owns it.  A wrong argtypes entry raises nothing when
it is called -- it truncates a stride or a pointer -- so this is where it is caught."""
import importlib
import re

import pytest

from pylbl_amd import abi
from tests import abi_header


@pytest.fixture(scope="module")
def lib():
    """liblbl_amd.so, built and loaded as tests/test_host_logic.py does; no GPU call is made."""
    import __graft_entry__
    __graft_entry__.build()
    return abi.library()


def test_the_header_declares_sixty_functions():
    """Every `name(` the header's code holds is a declaration the parser understood."""
    assert len(abi_header.DECLARATIONS) == 60
    assert set(re.findall(r"\b(lbl_\w+|absorption)\s*\(", abi_header.CODE)) == \
        set(abi_header.DECLARATIONS)
    assert abi_header.parameters_of("lbl_version") == []
    assert abi_header.DECLARATIONS["lbl_stream"][0] == "void *"
    assert abi_header.DECLARATIONS["lbl_last_error"][0] == "const char *"


def test_one_prototype_per_declaration_in_the_header_order():
    assert set(abi.PROTOTYPES) == set(abi_header.DECLARATIONS)
    assert list(abi.PROTOTYPES) == list(abi_header.DECLARATIONS)
    assert abi.EXPORTED_SYMBOLS == tuple(abi.PROTOTYPES)
    assert set(abi.RESULT_TYPES) == {"lbl_last_error", "lbl_stream", "lbl_version"}


@pytest.mark.parametrize("name", list(abi_header.DECLARATIONS))
def test_prototype_matches_its_declaration(lib, name):
    abi_header.check_argtypes(name)


def test_band_descriptor_is_struct_lbl_band():
    members = abi_header.band_members()
    assert [name for name, _ in members] == ["kind", "size", "lower_bound", "resolution", "column"]
    assert len(abi.BandDescriptor._fields_) == len(members)
    for (name, kind), (expected_name, expected) in zip(abi.BandDescriptor._fields_, members):
        assert name == expected_name
        if hasattr(expected, "_length_"):
            assert (kind._type_, kind._length_) == (expected._type_, expected._length_), name
        else:
            assert kind is expected, name


# #defines that pylbl_amd/abi.py does not mirror: those mirrored elsewhere, with the module that
# owns the mirror (its attribute is the attribute prefix and the rest of the name), and those that
# nothing in the package reads.  A new #define is mirrored in abi.py or entered here.
ELSEWHERE = (
    # (defines that start with, module, attribute prefix)
    ("LBL_BAND_", "pylbl_amd.mt_ckd", ""),                 # the band formulas of the continua
    ("LBL_INSTRUMENT_", "pylbl_amd.instrument", ""),       # the line-shape codes
    ("LBL_PLANCK_", "pylbl_amd.paths", "PLANCK_"),         # C1, C2
    ("LBL_SOLAR_", "pylbl_amd.paths", "SOLAR_"),           # the Sun's temperature, solid angle
)
NOT_MIRRORED = {
    # Status codes nobody reads: callers test for LBL_OK and raise with lbl_last_error's message.
    "LBL_ERROR", "LBL_BAD_ARGUMENT", "LBL_NO_DEVICE", "LBL_OUT_OF_RANGE",
    # Checked by the C entry alone.
    "LBL_MAX_PEDESTAL_CUT_OFF",
}


def test_every_define_is_mirrored_or_listed():
    defined = abi_header.defines()
    assert len(defined) >= 60 and "LBL_AMD_H_" not in defined
    mirrored = 0
    for name, text in defined.items():
        if name in NOT_MIRRORED:
            continue
        owner = [(module, attribute + name[len(prefix):])
                 for prefix, module, attribute in ELSEWHERE if name.startswith(prefix)]
        if owner:
            (module, attribute), = owner
            assert getattr(importlib.import_module(module), attribute) == float(text), name
            continue
        assert re.fullmatch(r"0x[0-9a-fA-F]+|\d+", text), f"{name} {text}: no integer, no owner"
        attribute = name if name == "LBL_OK" else name[len("LBL_"):]
        assert hasattr(abi, attribute), f"{name} has no mirror in pylbl_amd/abi.py"
        assert getattr(abi, attribute) == int(text, 0), name
        mirrored += 1
    assert mirrored >= 38
    assert abi.RANGE_POLICIES == {"reference": abi.RANGE_REFERENCE, "skip": abi.RANGE_SKIP}


def test_engine_module_still_resolves_what_callers_read_from_it():
    from pylbl_amd import device_memory, engine
    for name in ("EXPORTED_SYMBOLS", "library", "read_line_table", "LBL_OK",
                 "PATH_JACOBIAN_OUTPUTS") + \
            tuple(x for x in vars(abi) if x.startswith(("TABLE_", "PATH_", "VMR_"))):
        assert getattr(engine, name) is getattr(abi, name), name
    for name in ("DeviceSpectra", "DevicePool"):
        assert getattr(engine, name) is getattr(device_memory, name), name
    assert engine.default_engine.__module__ == engine.Engine.__module__ == "pylbl_amd.engine"
