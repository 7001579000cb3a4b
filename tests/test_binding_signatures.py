"""include/pcbenv.h and pcbenv/_lib.py declare the C ABI twice: this keeps the two in agreement, type by type, for every
prototype (argument count, every argument's ctypes type, the return type) and every struct (member names, member types
and -- with a C compiler at hand -- size and every member's offset).  No compute call is made."""
import ctypes as C
import re
import shutil

import pytest

import abi_header
import model_harness
from pcbenv import _lib

SCALARS = {"int": C.c_int, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16, "int32_t": C.c_int32,
           "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
# the ctypes Structure of every struct of the header, by the header's name (PcbenvTreeRequest <-> pcbenv_tree_request)
STRUCTURES = {re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower(): cls for name, cls in vars(_lib).items()
              if isinstance(cls, type) and issubclass(cls, C.Structure) and cls is not C.Structure}
PROTOTYPES = abi_header.prototypes()


def _pointer_ok(ctype: str, bound) -> bool:
    """A C pointer is bound as c_void_p or as a POINTER to its pointee's type: the Structure of a struct, the ctypes scalar
    of a scalar, c_void_p where the pointee is itself a pointer or an opaque handle."""
    if bound is C.c_void_p:
        return True
    pointee = re.sub(r"\bconst\b", "", ctype.rstrip()[:-1]).strip()
    if pointee.endswith("*") or pointee in ("pcbenv", "pcbenv_instgen", "void"):
        want = C.c_void_p
    else:
        want = STRUCTURES.get(pointee) or SCALARS.get(pointee)
    return want is not None and bound is C.POINTER(want)


def _type_ok(ctype: str, bound) -> bool:
    return _pointer_ok(ctype, bound) if ctype.endswith("*") else bound is SCALARS[ctype]


def test_the_parser_sees_the_whole_header():
    names = [name for _, name, _ in PROTOTYPES]
    assert len(names) == len(set(names)) == 40 and set(names) == set(_lib.EXPORTS)
    assert set(abi_header.structs()) == set(STRUCTURES) and len(STRUCTURES) == 6
    assert ("int", "pcbenv_create", [("const pcbenv_config *", "cfg"), ("int", "device"), ("pcbenv **", "out")]) in PROTOTYPES
    assert ("int", "pcbenv_abi_version", []) in PROTOTYPES
    assert ("pcbenv_instgen *const *", "streams") in dict((n, p) for _, n, p in PROTOTYPES)["pcbenv_instgen_next_batch"]


@pytest.mark.parametrize("ret, name, params", PROTOTYPES, ids=[name for _, name, _ in PROTOTYPES])
def test_the_binding_has_the_prototype(ret, name, params):
    f = getattr(_lib.load(), name)
    argtypes = list(f.argtypes or [])  # never set: ctypes converts whatever it is given, which is right for `(void)` alone
    assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
    for i, ((ctype, pname), bound) in enumerate(zip(params, argtypes)):
        assert _type_ok(ctype, bound), f"{name}: parameter {i}, `{ctype} {pname}`, is bound as {bound.__name__}"
    if ret == "void":
        assert f.restype is None, name
    elif ret == "const char *":
        assert f.restype is C.c_char_p, name
    else:
        assert _type_ok(ret, f.restype), f"{name} returns `{ret}` and is bound as returning {f.restype}"


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_the_structure_has_the_members(name):
    members, fields = abi_header.structs()[name], STRUCTURES[name]._fields_
    assert [n for n, _ in fields] == [n for _, n in members]
    for (ctype, member), (_, bound) in zip(members, fields):
        assert _type_ok(ctype, bound), f"{name}.{member}: `{ctype}` is bound as {bound.__name__}"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_every_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset of every struct as a C compiler lays include/pcbenv.h out."""
    got = {}
    for name, members in abi_header.structs().items():
        offsets, size = model_harness.layout("pcbenv.h", name, [m for _, m in members])
        got[name] = dict(offsets, sizeof=size)
    want = {name: dict({n: getattr(cls, n).offset for n, _ in cls._fields_}, sizeof=C.sizeof(cls)) for name, cls in STRUCTURES.items()}
    assert got == want
