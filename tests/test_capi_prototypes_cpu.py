"""The ctypes table of qpwcnet_amd/_hip.py against the prototypes of include/qpwc.h: same names, same order, same
types.  A wrong width in the table (`int` for `int64_t`) corrupts an argument silently; nothing else would notice.
Needs no library and no GPU."""
import ctypes
import os
import re

from qpwcnet_amd import _hip

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc.h")

# every parameter spelling and return type the header uses
PARAM_TYPES = {
    "const void*": ctypes.c_void_p,
    "void*": ctypes.c_void_p,
    "const void* const*": ctypes.POINTER(ctypes.c_void_p),
    "void* const*": ctypes.POINTER(ctypes.c_void_p),
    "const int*": ctypes.POINTER(ctypes.c_int),
    "const int64_t*": ctypes.POINTER(ctypes.c_int64),
    "int": ctypes.c_int,
    "float": ctypes.c_float,
    "int64_t": ctypes.c_int64,
    "long long": ctypes.c_longlong,
}
RETURN_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}


def parse_header(path=HEADER):
    """[(name, return spelling, [parameter spellings])] for every qpwc_* prototype, in the header's order."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    protos = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(qpwc_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        spellings = []
        for p in params.split(","):
            p = " ".join(p.split())
            if p == "void":
                continue
            # drop the parameter's name: the last identifier
            p = re.sub(r"\s*\b[A-Za-z_]\w*$", "", p)
            spellings.append(re.sub(r"\s*\*", "*", p).replace("*const", "* const"))
        protos.append((name, ret, spellings))
    return protos


def same_ctype(a, b):
    """Equal as the ABI sees them: ctypes spells int64_t as c_long and long long as c_longlong on LP64; both are one
    signed 64-bit integer.  Pointers compare by what they point to."""
    if a is b:
        return True
    if hasattr(a, "contents") and hasattr(b, "contents"):
        return same_ctype(a._type_, b._type_)
    ints = "bhilq"
    if isinstance(getattr(a, "_type_", None), str) and isinstance(getattr(b, "_type_", None), str):
        return (a._type_ in ints and b._type_ in ints and ctypes.sizeof(a) == ctypes.sizeof(b))
    return False


def mismatches(table, protos=None):
    """Every disagreement between a name -> (restype, argtypes) table and the header, as text."""
    protos = parse_header() if protos is None else protos
    bad = []
    if list(table) != [name for name, _, _ in protos]:
        bad.append("names or order differ: table only {}, header only {}".format(
            sorted(set(table) - {n for n, _, _ in protos}), sorted({n for n, _, _ in protos} - set(table))))
    for name, ret, params in protos:
        if name not in table:
            continue
        restype, argtypes = table[name]
        if not same_ctype(restype, RETURN_TYPES[ret]):
            bad.append("{}: returns {}, table has {}".format(name, ret, restype))
        if len(argtypes) != len(params):
            bad.append("{}: {} parameters, table has {}".format(name, len(params), len(argtypes)))
            continue
        for i, (spelling, have) in enumerate(zip(params, argtypes)):
            if not same_ctype(have, PARAM_TYPES[spelling]):
                bad.append("{}: parameter {} is `{}`, table has {}".format(name, i, spelling, have))
    return bad


def test_header_parses_into_known_spellings():
    protos = parse_header()
    assert len(protos) == 77
    assert len({name for name, _, _ in protos}) == len(protos)
    assert {ret for _, ret, _ in protos} == set(RETURN_TYPES)
    assert {p for _, _, params in protos for p in params} == set(PARAM_TYPES)


def test_table_matches_header():
    assert mismatches(_hip.PROTOTYPES) == []
    assert tuple(_hip.SYMBOLS) == tuple(name for name, _, _ in parse_header())


def test_a_wrong_width_is_caught():
    table = dict(_hip.PROTOTYPES)
    restype, argtypes = table["qpwc_device_copy"]
    table["qpwc_device_copy"] = (restype, [ctypes.c_int if t is ctypes.c_int64 else t for t in argtypes])
    assert mismatches(table) == ["qpwc_device_copy: parameter 2 is `int64_t`, table has {}".format(ctypes.c_int)]
    table["qpwc_device_copy"] = (ctypes.c_int64, argtypes)
    assert mismatches(table) == ["qpwc_device_copy: returns int, table has {}".format(ctypes.c_int64)]
