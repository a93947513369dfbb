"""``include/imx.h`` read once: the header is the only place the ABI is written, and the ctypes binding (``_lib.py``), the plan
constants (``plan.py``) and the event op codes (``events.py``) are derived from the four tables below.

This is no C parser.  It reads the subset the header uses -- integer ``#define IMX_*``, ``enum``, ``typedef struct`` of scalars, pointers,
arrays and earlier ABI structs, opaque ``typedef struct x x_t;``, ``typedef void* x_t;`` and function declarations -- and raises
``AbiError`` with the header line for anything else: a header edit it cannot read fails at import instead of binding wrongly."""

from __future__ import annotations

import ctypes
import os
import re
from typing import NamedTuple

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "imx.h"))

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "uint8_t": ctypes.c_uint8, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
_POINTEES = ("void", "char", "uint32_t")  # read only behind a pointer
_DECL = re.compile(r"(?:const\s+)?(\w+)((?:\s*\*(?:\s*const\b)?)*)\s*(\w*)\s*(?:\[\s*(\w+)\s*\])?")


class AbiError(ValueError):
    pass


class CType(NamedTuple):
    """A type as the header spells it: ``const float* x`` is ``("float", 1, 0)``, ``float ranges[24]`` is ``("float", 0, 24)``."""

    base: str
    ptr: int = 0
    dim: int = 0


def ctype(t: CType, classes: dict, ret: bool = False):
    """The ctypes type of ``t``.  ``classes``: typedef name -> ``ctypes.Structure`` of the ABI structs.  A pointer to one of them is
    ``POINTER(class)``, a returned ``const char*`` is ``c_char_p``, every other pointer is ``c_void_p``."""
    if ret and t == ("char", 1, 0):
        return ctypes.c_char_p
    if ret and t == ("void", 0, 0):
        return None
    if t.ptr:
        c = ctypes.POINTER(classes[t.base]) if t.ptr == 1 and t.base in classes else ctypes.c_void_p
    else:
        c = _SCALARS.get(t.base) or classes[t.base]
    return c * t.dim if t.dim else c


def parse(text: str, path: str = "imx.h", known_defines: dict | None = None):
    """``(DEFINES, ENUMS, STRUCTS, FUNCTIONS)`` of a header text.  ``known_defines``: the ``#define IMX_*`` of the header that includes
    this one (array sizes may use them); they are not returned."""
    defines, enums, structs, functions, opaque, handles = dict(known_defines or {}), {}, {}, {}, set(), set()

    def fail(pos: int, msg: str):
        raise AbiError(f"{path}:{code.count(chr(10), 0, pos) + 1}: {msg}")

    def split(lo: int, hi: int, sep: str, terminated: bool):
        """(position, text) of the pieces of code[lo:hi] that ``sep`` separates outside any bracket."""
        depth, start = 0, lo

        def piece(end):
            s = code[start:end]
            return start + len(s) - len(s.lstrip()), s.strip()

        for m in re.compile(r"[(){}\[\]%s]" % sep).finditer(code, lo, hi):
            if m.group() == sep:
                if depth == 0:
                    yield piece(m.start())
                    start = m.end()
            else:
                depth += 1 if m.group() in "({[" else -1
                if depth < 0:
                    fail(m.start(), f"unbalanced '{m.group()}'")
        if piece(hi)[1]:
            if terminated or depth:
                fail(piece(hi)[0], f"a declaration that does not end (no closing '{'}' if depth else sep}')")
            yield piece(hi)

    def integer(pos: int, s: str) -> int:
        try:
            return defines[s] if s in defines else int(s, 0)
        except ValueError:
            fail(pos, f"'{s}' is neither an integer literal nor a #define above")

    def decl(pos: int, s: str, named: bool, base: str | None = None) -> tuple[str, CType]:
        """``const float* x``, ``float ranges[24]``, a bare return type (``named`` false), or a further name of a multi-declarator line
        (``base``: the type its first declarator gave)."""
        m = _DECL.fullmatch(s if base is None else f"{base} {s}")
        if not m or bool(m.group(3)) != named or (base is not None and m.group(2)):
            what = "a bit-field" if ":" in s else "a function pointer" if "(" in s else "a nested struct or union" if "{" in s else "no declaration of the subset read here"
            fail(pos, f"'{s}' is {what}")
        b, ptr = m.group(1), m.group(2).count("*")
        if b in handles:
            b, ptr = "void", ptr + 1
        if not (b in _SCALARS or b in structs or (ptr and (b in opaque or b in _POINTEES)) or (b == "void" and not named)):
            fail(pos, f"type '{b}' is opaque: only a pointer to it can be passed" if b in opaque else f"unknown type '{b}'")
        return m.group(3), CType(b, ptr, integer(pos, m.group(4)) if m.group(4) else 0)

    # comments out (newlines kept: a position gives its header line), then the preprocessor lines
    code = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)
    lines, guard, cxx, pos = code.split("\n"), None, False, 0
    for i, line in enumerate(lines):
        if line.lstrip().startswith("#"):
            d = line.strip()[1:].split()
            if d[:1] == ["ifndef"] and guard is None and len(d) == 2:
                guard = d[1]
            elif d == ["ifdef", "__cplusplus"]:
                cxx = True
            elif d == ["endif"]:
                cxx = False
            elif d[:1] == ["define"] and len(d) == 3 and d[1].startswith("IMX_"):
                defines[d[1]] = integer(pos, d[2])
            elif not (d[:1] == ["include"] or d == ["define", guard]):
                fail(pos, f"'{line.strip()}': only the include guard, #include, #ifdef __cplusplus and integer #define IMX_* are read")
        if cxx or line.lstrip().startswith("#"):  # (cxx: the extern "C" braces)
            lines[i] = ""
        pos += len(line) + 1
    code = "\n".join(lines)

    for pos, s in split(0, len(code), ";", True):
        if m := re.fullmatch(r"typedef\s+struct\s+\w+\s+(\w+)", s):
            opaque.add(m.group(1))
        elif m := re.fullmatch(r"typedef\s+void\s*\*\s*(\w+)", s):
            handles.add(m.group(1))
        elif m := re.fullmatch(r"enum\s+(\w+)\s*\{(.*)\}", s, re.S):
            members, nxt = {}, 0
            for p, item in split(pos + m.start(2), pos + m.end(2), ",", False):
                name, eq, val = (x.strip() for x in item.partition("="))
                if not re.fullmatch(r"\w+", name):
                    fail(p, f"'{item}' is no enum member")
                members[name] = nxt = integer(p, val) if eq else nxt
                nxt += 1
            enums[m.group(1)] = members
        elif m := re.fullmatch(r"typedef\s+struct\s+\w+\s*\{(.*)\}\s*(\w+)", s, re.S):
            fields = []
            for p, line in split(pos + m.start(1), pos + m.end(1), ";", True):
                first, *more = split(p, p + len(line), ",", False)
                fields.append(decl(*first, named=True))
                fields += [decl(q, x, named=True, base=fields[-1][1].base) for q, x in more]
            structs[m.group(2)] = fields
        elif m := re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", s, re.S):
            params = [] if m.group(3).strip() == "void" else [decl(p, x, named=True) for p, x in split(pos + m.start(3), pos + m.end(3), ",", False)]
            if any(t.dim for _, t in params):
                fail(pos, f"{m.group(2)}: an array parameter")
            functions[m.group(2)] = (decl(pos, m.group(1).strip(), named=False)[1], [t for _, t in params], [n for n, _ in params])
        else:
            fail(pos, f"'{s.split(chr(10))[0]}' is no declaration of the subset read here")
    return {k: v for k, v in defines.items() if k not in (known_defines or {})}, enums, structs, functions


try:
    with open(HEADER) as _f:
        DEFINES, ENUMS, STRUCTS, FUNCTIONS = parse(_f.read(), HEADER)
    # imx_osc_struct.h, which imx.h includes for the one struct it declares but does not define (imx_osc_t)
    OSC_HEADER = os.path.join(os.path.dirname(HEADER), "imx_osc_struct.h")
    with open(OSC_HEADER) as _f:
        _, _, OSC_STRUCTS, _ = parse(_f.read(), OSC_HEADER, DEFINES)
    # imx_orch_manip.h, likewise: imx_orch_manip_t and the imx_weight_term_t it holds (imx_reset_orchestrate_manip)
    MANIP_HEADER = os.path.join(os.path.dirname(HEADER), "imx_orch_manip.h")
    with open(MANIP_HEADER) as _f:
        _manip_defines, _, MANIP_STRUCTS, _ = parse(_f.read(), MANIP_HEADER, DEFINES)
    DEFINES.update(_manip_defines)  # IMX_ORCH_MAX_WEIGHT_TERMS
    # imx_pretrained_policy_struct.h, likewise: imx_pretrained_policy_t (imx_pretrained_policy)
    POLICY_HEADER = os.path.join(os.path.dirname(HEADER), "imx_pretrained_policy_struct.h")
    with open(POLICY_HEADER) as _f:
        _policy_defines, _, POLICY_STRUCTS, _ = parse(_f.read(), POLICY_HEADER, DEFINES)
    DEFINES.update(_policy_defines)  # IMX_PP_MAX_LAYERS
    # imx_pose2d_struct.h, likewise: imx_pose2d_command_t (imx_pose2d_command, imx_reset_orchestrate_pose2d)
    POSE2D_HEADER = os.path.join(os.path.dirname(HEADER), "imx_pose2d_struct.h")
    with open(POSE2D_HEADER) as _f:
        _, _, POSE2D_STRUCTS, _ = parse(_f.read(), POSE2D_HEADER, DEFINES)
    # imx_inhand_command_struct.h, likewise: imx_inhand_command_t (imx_inhand_command)
    INHAND_HEADER = os.path.join(os.path.dirname(HEADER), "imx_inhand_command_struct.h")
    with open(INHAND_HEADER) as _f:
        _, _, INHAND_STRUCTS, _ = parse(_f.read(), INHAND_HEADER, DEFINES)
    # imx_object_state.h, likewise: imx_object_state_t (imx_plan_bind_object_state)
    OBJECT_STATE_HEADER = os.path.join(os.path.dirname(HEADER), "imx_object_state.h")
    with open(OBJECT_STATE_HEADER) as _f:
        _, _, OBJECT_STATE_STRUCTS, _ = parse(_f.read(), OBJECT_STATE_HEADER, DEFINES)
    # imx_articulation_state.h, likewise: imx_articulation_state_t (imx_plan_bind_articulation_state)
    ARTICULATION_STATE_HEADER = os.path.join(os.path.dirname(HEADER), "imx_articulation_state.h")
    with open(ARTICULATION_STATE_HEADER) as _f:
        _, _, ARTICULATION_STATE_STRUCTS, _ = parse(_f.read(), ARTICULATION_STATE_HEADER, DEFINES)
    # imx_orch_articulation.h, likewise: imx_orch_articulation_t (imx_reset_orchestrate_scene)
    ORCH_ARTICULATION_HEADER = os.path.join(os.path.dirname(HEADER), "imx_orch_articulation.h")
    with open(ORCH_ARTICULATION_HEADER) as _f:
        _, _, ORCH_ARTICULATION_STRUCTS, _ = parse(_f.read(), ORCH_ARTICULATION_HEADER, DEFINES)
    # imx_normalization_struct.h, likewise: imx_norm_group_t (imx_empirical_normalization_update), imx_infer_norm_t (imx_mlp_infer_act2n)
    NORMALIZATION_HEADER = os.path.join(os.path.dirname(HEADER), "imx_normalization_struct.h")
    with open(NORMALIZATION_HEADER) as _f:
        _, _, NORMALIZATION_STRUCTS, _ = parse(_f.read(), NORMALIZATION_HEADER, DEFINES)
    # imx_ray_caster_struct.h, likewise: imx_ray_caster_t (imx_ray_caster)
    RAY_CASTER_HEADER = os.path.join(os.path.dirname(HEADER), "imx_ray_caster_struct.h")
    with open(RAY_CASTER_HEADER) as _f:
        _, _, RAY_CASTER_STRUCTS, _ = parse(_f.read(), RAY_CASTER_HEADER, DEFINES)
    # imx_imu_struct.h, likewise: imx_imu_t (imx_imu, imx_plan_bind_imu)
    IMU_HEADER = os.path.join(os.path.dirname(HEADER), "imx_imu_struct.h")
    with open(IMU_HEADER) as _f:
        _, _, IMU_STRUCTS, _ = parse(_f.read(), IMU_HEADER, DEFINES)
except OSError as e:
    raise AbiError(f"the ABI header {HEADER} cannot be read ({e}): the whole binding is derived from it") from e
