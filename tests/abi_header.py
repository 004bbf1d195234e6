"""include/lbl_amd.h as the tests read it: every function declaration, struct lbl_band and the
#defines, parsed once, and the one comparison of a declaration with its ctypes prototype
(pylbl_amd/abi.py) that tests/test_abi_host.py runs over the whole header and the per-feature host
tests run on their own entries."""
import ctypes
from ctypes import c_char_p, c_double, c_int32, c_int64, c_void_p
from pathlib import Path
import re

from pylbl_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "lbl_amd.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)        # the header without its comments

SCALARS = {"double": c_double, "int32_t": c_int32, "int": c_int32, "int64_t": c_int64}
POINTEES = dict(SCALARS, lbl_band=abi.BandDescriptor)
RESULTS = {"int": c_int32, "const char *": c_char_p, "void *": c_void_p}


def _squeeze(text):
    return re.sub(r"\s+", " ", text).strip()


def _declarations():
    """{function: (result type, [parameter, ...])} in the header's order; (void) is no parameter."""
    found = {}
    for result, name, inside in re.findall(
            r"^(int|const char \*|void \*)\s*(lbl_\w+|absorption)\s*\(([^)]*)\)\s*;", CODE, re.M):
        assert name not in found, name
        inside = _squeeze(inside)
        found[name] = (result, [] if inside == "void" else [_squeeze(p) for p in
                                                            inside.split(",")])
    return found


DECLARATIONS = _declarations()


def parameters_of(name):
    """The parameters of the header's declaration of `name`, as it writes them, blanks squeezed."""
    assert name in DECLARATIONS, name
    return list(DECLARATIONS[name][1])


def defines():
    """{name: text of the value} of every #define LBL_* that has a value, in the header's order."""
    return dict(re.findall(r"^#define[ \t]+(LBL_\w+)[ \t]+(\S+)", CODE, re.M))


def band_members():
    """[(name, ctypes type)] of the members of struct lbl_band."""
    body = re.search(r"typedef struct lbl_band\s*\{([^}]*)\}\s*lbl_band;", CODE).group(1)
    members = []
    for base, name, length in re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?\s*;", body):
        members.append((name, SCALARS[base]*int(length) if length else SCALARS[base]))
    return members


def check_parameter(argtype, parameter, addresses=False):
    """One ctypes argument type against one parameter of the header.  A scalar needs its own
    type.  Anything with * or [ needs a pointer: c_void_p, c_char_p only for a char *, or
    POINTER(T) with T the pointee (c_void_p for a **); with `addresses` (entries whose callers
    pass plain addresses) nothing but c_void_p."""
    text = parameter.replace("const ", "")
    base, stars = text.split()[0], text.count("*")
    if stars == 0 and "[" not in text:
        assert argtype is SCALARS[base], parameter
        return
    if addresses:
        assert argtype is c_void_p, parameter
    if argtype is c_void_p:
        return
    if argtype is c_char_p:
        assert base == "char" and stars == 1, parameter
        return
    assert isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer), parameter
    assert argtype._type_ is (c_void_p if stars == 2 else POINTEES.get(base)), parameter


def check_argtypes(name, parameters=None, addresses=False):
    """The prototype of `name` in abi.PROTOTYPES, and what library() set on the loaded function,
    against `parameters` (default: the header's): count, every type, the result type."""
    result, declared = DECLARATIONS[name]
    parameters = declared if parameters is None else parameters
    assert name in abi.PROTOTYPES and name in abi.EXPORTED_SYMBOLS, name
    argtypes = abi.PROTOTYPES[name]
    assert len(argtypes) == len(parameters), name
    for argtype, parameter in zip(argtypes, parameters):
        check_parameter(argtype, parameter, addresses)
    assert (name in abi.RESULT_TYPES) == (result != "int"), name
    function = getattr(abi.library(), name)
    assert list(function.argtypes) == list(argtypes), name
    assert function.restype is abi.RESULT_TYPES.get(name, c_int32) is RESULTS[result], name
