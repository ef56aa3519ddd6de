"""The ctypes binding states the C ABI once, in native._SIGNATURES: that table, the VqArgs structure and the Python constants
are compared here with include/vq_mi355x.h type by type, and load() must bind exactly the table (host only)."""
from __future__ import annotations

import ctypes
import os
import re

import pytest

from vector_quantization import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
    "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
}


def _header() -> str:
    """The header without its comments."""
    text = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _ctype(base: str, stars: str):
    """The ctypes type of a C type: ``base`` without qualifiers, ``stars`` its pointer depth.  Unknown types fail the test."""
    base = " ".join(w for w in base.split() if w not in ("const", "struct"))
    if stars:
        return {"vq_args": ctypes.POINTER(native.VqArgs), "char": ctypes.c_char_p}.get(base, ctypes.c_void_p)
    if base not in SCALARS:
        pytest.fail(f"type {base!r} of the header has no ctypes mapping in this test")
    return SCALARS[base]


def _declarators(decl: str):
    """``const float *x`` or ``int64_t x_rs, x_hs`` -> [(name, ctypes type), ...]: the base type is shared, the stars are not."""
    first, *rest = [p.strip() for p in decl.split(",")]
    m = re.fullmatch(r"(.*?)(\**)\s*(\w+)", first, flags=re.S)
    assert m and m.group(1).strip(), f"cannot parse the declaration {decl!r}"
    base = m.group(1)
    found = [(m.group(3), _ctype(base, m.group(2)))]
    for piece in rest:
        m = re.fullmatch(r"(\**)\s*(\w+)", piece)
        assert m, f"cannot parse the declaration {decl!r}"
        found.append((m.group(2), _ctype(base, m.group(1))))
    return found


def header_prototypes() -> dict:
    """name -> (restype, argtypes) for every vq_* prototype of the header."""
    text = _header()
    protos = {}
    for m in re.finditer(r"((?:const\s+)?\w+)\s*(\**)\s*\b(vq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret, stars, name, params = m.groups()
        assert name not in protos, f"{name} is declared twice"
        params = params.strip()
        args = () if params in ("", "void") else tuple(_declarators(p)[0][1] for p in params.split(","))
        protos[name] = (_ctype(ret, stars), args)
    # no prototype may be left out: every vq_ name that is followed by a parenthesis was parsed
    assert set(protos) == set(re.findall(r"\b(vq_[a-z0-9_]+)\s*\(", text))
    return protos


def header_struct_fields():
    body = re.search(r"typedef\s+struct\s+vq_args\s*\{(.*?)\}\s*vq_args\s*;", _header(), flags=re.S).group(1)
    return [f for decl in body.split(";") if decl.strip() for f in _declarators(decl.strip())]


def header_constants() -> dict:
    """#define VQ_NAME value (an integer, possibly parenthesised or with a u suffix) -> {name: value}."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(VQ_\w+)\s+\(?(-?\d+)u?\)?", _header())}


def mismatches(protos: dict, table: dict) -> list:
    """Every way ``table`` (name -> (restype, argtypes)) disagrees with the header's prototypes, as readable lines."""
    found = [f"{n}: declared in the header, missing from the table" for n in sorted(set(protos) - set(table))]
    found += [f"{n}: in the table, not declared in the header" for n in sorted(set(table) - set(protos))]
    for name in sorted(set(protos) & set(table)):
        (want_ret, want_args), (ret, args) = protos[name], table[name]
        if ret is not want_ret:
            found.append(f"{name}: returns {want_ret.__name__}, the table says {getattr(ret, '__name__', ret)}")
        if len(args) != len(want_args):
            found.append(f"{name}: {len(want_args)} parameters, the table has {len(args)}")
            continue
        found += [f"{name}: parameter {i} is {w.__name__}, the table says {getattr(t, '__name__', t)}"
                  for i, (w, t) in enumerate(zip(want_args, args)) if t is not w]
    return found


def test_parser_sees_the_whole_header():
    protos = header_prototypes()
    assert len(protos) >= 60
    assert protos["vq_last_error"] == (ctypes.c_char_p, ())
    assert protos["vq_device_info"] == (ctypes.c_int, (ctypes.c_char_p, ctypes.c_size_t))
    assert protos["vq_quantize_f32"] == (ctypes.c_int, (ctypes.POINTER(native.VqArgs), ctypes.c_void_p))
    assert protos["vq_keys_init"] == (ctypes.c_int, (ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p))


def test_signature_table_matches_header():
    assert mismatches(header_prototypes(), native._SIGNATURES) == []
    assert native.EXPORTED_SYMBOLS == tuple(native._SIGNATURES)


def _corrupted():
    """(what was done, the name it was done to, the corrupted copy of the table)"""
    t = dict(native._SIGNATURES)
    ret, args = t["vq_keys_init"]
    assert args[1] is ctypes.c_int64
    yield "an int64_t narrowed to int", "vq_keys_init", {**t, "vq_keys_init": (ret, (args[0], ctypes.c_int, args[2]))}
    ret, args = t["vq_quantize_backward_f32"]
    yield "a stride parameter dropped", "vq_quantize_backward_f32", {**t, "vq_quantize_backward_f32": (ret, args[:-2] + args[-1:])}
    ret, args = t["vq_packed_floats"]
    assert ret is ctypes.c_int64
    yield "a return type changed", "vq_packed_floats", {**t, "vq_packed_floats": (ctypes.c_int, args)}
    yield "a name removed", "vq_lq_backward_f32", {k: v for k, v in t.items() if k != "vq_lq_backward_f32"}


@pytest.mark.parametrize("what,name,table", list(_corrupted()), ids=[c[0] for c in _corrupted()])
def test_comparison_reports_a_corrupted_table(what, name, table):
    found = mismatches(header_prototypes(), table)
    assert len(found) == 1 and found[0].startswith(name + ":"), (what, found)


def test_struct_matches_header():
    assert header_struct_fields() == list(native.VqArgs._fields_)


def test_constants_match_header():
    consts = header_constants()
    checked = 0
    for name, value in consts.items():
        if name.startswith("VQ_METRIC_"):
            py = name[len("VQ_METRIC_"):]
        elif name.startswith("VQ_F_"):
            py = name[len("VQ_"):]
        elif name == "VQ_E_UNSUPPORTED":
            py = "E_UNSUPPORTED"
        else:
            continue
        assert getattr(native, py) == value, f"{name} = {value} in the header, native.{py} = {getattr(native, py, None)}"
        checked += 1
    assert checked == 9  # two metrics, six flags, one error code


def test_binding_follows_the_table():
    if not os.path.exists(native.lib_path()):
        import __graft_entry__

        __graft_entry__.build()
    lib = native.load()
    for name, (restype, argtypes) in native._SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
