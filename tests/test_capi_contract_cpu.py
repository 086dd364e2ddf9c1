"""The argument validation of every entry point of libqpwc_hip.so, pinned case by case.

tests/golden/capi_contract.json records, for one valid call of each validating entry point and for many mutations of
it, the value the call returned and the text qpwc_last_error() held afterwards.  The test replays every case against
the in-tree library and asserts both are equal: a change of the boundary code (csrc/capi.hip) that rejects a valid
call, accepts an invalid one, or answers two defects in another order shows up here, on a machine without a GPU.

The pointers are offsets into one 16-byte aligned HOST buffer.  Validation only looks at their values; without a
device a call that passes it fails at the launch (QPWC_E_LAUNCH, "... no ROCm-capable device is detected"), which is
what the golden holds for every base tuple.  With a device such a call would launch on host memory, so the module
skips itself there.

The golden is never written from the code under test: `QPWC_HIP_LIB=<library of the parent commit> python
tests/test_capi_contract_cpu.py` writes it.  A new entry point adds a row to ENTRIES below (or to EXEMPT) and its
cases to the golden the same way, from a build that is known good.
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

if __name__ == "__main__":  # run as a script (which writes the golden) the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qpwcnet_amd import _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_contract.json")
SLOT = 1 << 20          # operand k of a call lives at offset k * SLOT: far larger than any operand at these shapes
N_SLOTS = 24
BIG = 1 << 30           # an extent that trips the 32-bit and launch-grid guards
_PVP, _PI, _PI64 = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)


# ---- the case table: one row per validating entry point, one item per argument -------------------------------------
# Each item is (kind, base value, bad values, tag).  kind: "in" / "out" a pointer (base value: its slot), "ins" /
# "outs" an array of pointers, "n" an integer or float, "ns" an array of integers, "s" the stream (always NULL).
# The tag names the check a bad value aims at; a pair of mutations is formed only across different tags.

def IN(slot):
    return ("in", slot * SLOT, (), None)


def OUT(slot):
    return ("out", slot * SLOT, (), None)


def INS(*slots):
    return ("ins", [s * SLOT for s in slots], (), None)


def OUTS(*slots):
    return ("outs", [s * SLOT for s in slots], (), None)


def N(base, *bad, tag="shape"):
    """A scalar: 0 and -1 (an extent that is zero or negative) and every listed bad value, where they differ from base."""
    return ("n", base, tuple(v for v in (0, -1) + bad if v != base), tag)


def R(base, *bad, tag="range"):
    return ("n", base, bad, tag)


def NS(base, *bad, tag="shape"):
    return ("ns", list(base), (0, -1) + bad, tag)


def LAY(base=0):
    return N(base, 7, tag="layout")


def DT(base=0):
    return N(base, 9, 1 - base, tag="dtype")


S = ("s", None, (), None)
B1, H2, W2 = N(1), N(2), N(2)
SEP_SRC = (INS(0, 1), NS([4, 4], 3), NS([4, 4], 2, 6, tag="stride"), N(2, 4), N(0, 4))
CONV = (IN(0), IN(1), IN(2), OUT(3))

ENTRIES = {
    "qpwc_layout_transpose_fwd": [IN(0), OUT(1), B1, H2, W2, N(4), LAY(), DT(), S],
    "qpwc_copy_pixels_fwd": [IN(0), OUT(1), B1, H2, W2, N(4, 3), NS([16, 8, 4], 2, 6, tag="stride"),
                             NS([16, 8, 4], 2, 6, tag="stride"), DT(), S],
    "qpwc_device_copy": [IN(0), OUT(1), N(64, 24, 1 << 41), S],
    "qpwc_cost_volume_fwd": [IN(0), IN(1), OUT(2), B1, H2, W2, N(4), N(1, 17, tag="range"), LAY(), DT(), R(0.1), S],
    "qpwc_cost_volume_fwd_strided": [IN(0), IN(1), OUT(2), B1, H2, W2, N(4), N(1, 17, tag="range"), DT(), R(0.1),
                                     N(12, 8, tag="stride"), N(0, 4, tag="stride"), S],
    "qpwc_warp_fwd": [IN(0), IN(1), OUT(2), B1, N(2, 1), N(2, 1), N(4), N(0, 8, 7), LAY(), DT(), N(0, 5, 1, tag="mode"),
                      S],
    "qpwc_cost_volume_bwd": [IN(0), IN(1), IN(2), IN(3), OUT(4), OUT(5), B1, H2, W2, N(4), N(1, 17, tag="range"), DT(),
                             R(0.1, -0.5), S],
    "qpwc_warp_bwd_workspace_floats": [B1, H2, W2, N(4), DT()],
    "qpwc_warp_bwd": [IN(0), IN(1), IN(2), OUT(3), OUT(4), OUT(5), B1, N(2, 1), N(2, 1), N(4), DT(),
                      N(0, 5, 1, tag="mode"), S],
    "qpwc_loss_workspace_floats": [N(0, 4, 3, tag="mode"), B1, N(4), N(4), N(2, 3), NS([2, 1], 3), NS([2, 1], 3),
                                   N(2, 9)],
    "qpwc_loss_fwd": [N(0, 4, 3, tag="mode"), R(0.1, -1.0), R(0.0), IN(0), B1, N(4), N(4), N(2, 3), LAY(), INS(1, 2),
                      NS([2, 1], 3), NS([2, 1], 3), NS([0, 0], 9, 1, tag="dtype"), N(2, 9), OUT(3), OUTS(4, 5),
                      OUTS(6, 7), OUT(8), S],
    "qpwc_loss_fwd_kernel": [N(0, 4, 3, tag="mode"), IN(0), B1, N(32), N(32), N(2, 3), NS([16, 8], 3), NS([16, 8], 3),
                             N(2, 9)],
    "qpwc_loss_bwd": [INS(0, 1), IN(2), OUTS(3, 4), NS([8, 2]), NS([0, 0], 9, 1, tag="dtype"), N(2, 9), S],
    "qpwc_augment_workspace_floats": [B1, H2, N(2, BIG)],
    "qpwc_augment_fwd": [IN(0), N(0, 9, 2, 1, tag="dtype"), IN(1), B1, N(4, BIG), N(4), IN(2), IN(3), H2, W2,
                         N(1, 4, 3, tag="mode"), LAY(), OUT(4), OUT(5), OUT(6), S],
    "qpwc_augment_fwd_kernel": [B1, H2, W2, IN(0), IN(1)],
    "qpwc_warp_cost_volume_fwd": [IN(0), IN(1), IN(2), OUT(3), B1, N(2, 1), N(2, 1), N(4), N(4, 17, tag="range"), DT(),
                                  R(0.1), N(84, 80, tag="stride"), N(0, 4, tag="stride"), S],
    "qpwc_cost_volume_kernel": [B1, H2, W2, N(4), N(4, 17, tag="range"), LAY(), DT(), N(84), N(1)],
    "qpwc_epe_fwd": [IN(0), IN(1), OUT(2), OUT(3), B1, H2, W2, LAY(), S],
    "qpwc_epe_multi_fwd": [INS(0, 1), INS(2, 3), NS([4, 4]), NS([0, 0], 3, 2), N(2, 9), OUT(4), OUT(5), S],
    "qpwc_epe_multi_mixed_fwd": [INS(0, 1), INS(2, 3), NS([4, 4]), NS([0, 0], 3, 2), NS([0, 1], 9, tag="dtype"),
                                 N(2, 9), OUT(4), OUT(5), S],
    "qpwc_cost_volume_to_flow_fwd": [IN(0), OUT(1), B1, H2, W2, N(9), N(12, 8, tag="stride"), LAY(), DT(), S],
    "qpwc_dwconv3x3_fwd": [INS(0, 1), NS([4, 4], tag="stride"), NS([4, 4], 2, tag="stride"), N(2, 4), N(0, 1), IN(2),
                           OUT(3), B1, H2, W2, DT(), S],
    "qpwc_sepconv3x3_fwd": [*SEP_SRC, IN(2), IN(3), IN(4), OUT(5), B1, H2, W2, N(16, 8, 24, 256), S],
    "qpwc_sepconv3x3_bwd_workspace_floats": [B1, N(2, BIG), W2, N(8, (1 << 20) + 1), N(16, 8, 24, 256)],
    "qpwc_sepconv3x3_bwd": [*SEP_SRC, IN(2), IN(3), IN(4), IN(5), OUTS(6, 7), OUT(8), OUT(9), OUT(10), OUT(11), B1,
                            N(2, BIG), W2, N(16, 8, 24, 256), S],
    "qpwc_sepconv3x3_x3_fwd": [*SEP_SRC, IN(2), IN(3), IN(4), OUT(5), B1, H2, W2, N(16, 8, 24, 256), S],
    "qpwc_sepconv3x3_f16_fwd": [*SEP_SRC, IN(2), IN(3), IN(4), OUT(5), B1, N(2, BIG), W2, N(16, 8, 24, 256), S],
    "qpwc_flow_head_fwd": [IN(0), IN(1), OUT(2), B1, H2, W2, R(1.0), DT(), LAY(), S],
    "qpwc_flow_head_stats_workspace_floats": [B1, N(2, BIG), W2],
    "qpwc_flow_head_stats_fwd": [IN(0), IN(1), IN(2), IN(3), IN(4), IN(5), OUT(6), OUT(7), R(0.9, -0.1, 1.5),
                                 R(0.001, 0.0, -1.0), OUT(8), OUT(9), OUT(10), B1, N(2, BIG), W2, S],
    "qpwc_flow_head_bwd_workspace_floats": [B1, N(2, BIG), W2],
    "qpwc_flow_head_bwd": [IN(0), IN(1), IN(2), R(0.001, 0.0, -1.0), N(1), R(1.0), IN(3), OUT(4), OUT(5), OUT(6),
                           OUT(7), OUT(8), OUT(9), OUT(10), B1, N(2, BIG), W2, S],
    "qpwc_pointwise_bias_fwd": [IN(0), IN(1), IN(2), OUT(3), N(4, 1 << 31), N(8), N(16, 8, 24, 512), S],
    "qpwc_flow_head_up_fwd": [IN(0), IN(1), OUT(2), OUT(3), OUT(4), B1, N(2, 1 << 28), W2, R(1.0), R(2.0),
                              N(1, 9, 0, tag="dtype"), S],
    "qpwc_optflow_tail_fwd": [IN(0), IN(1), IN(2), IN(3), IN(4), IN(5), IN(6), IN(7), OUT(8), B1, H2, W2, R(1.0),
                              N(0, 1), LAY(), S],
    "qpwc_bias_mish_fwd": [IN(0), IN(1), N(4), N(4, 3), DT(), S],
    "qpwc_bias_mish_pad_fwd": [IN(0), IN(1), OUT(2), B1, H2, W2, N(4, 3), N(1), N(1), N(4, 2, 6, tag="stride"), DT(),
                               S],
    "qpwc_split_frames_pad_fwd": [IN(0), OUT(1), B1, H2, W2, N(1), N(1), DT(), S],
    "qpwc_upsample2x_flow_fwd": [IN(0), OUT(1), B1, H2, W2, R(2.0), DT(), LAY(), LAY(), S],
    "qpwc_upsample2x_flow_bwd": [IN(0), OUT(1), B1, N(2, (1 << 29) + 1), W2, R(2.0), S],
    "qpwc_invert_flow_fwd": [IN(0), OUT(1), B1, H2, W2, LAY(), DT(), S],
    "qpwc_occlusion_fwd": [IN(0), OUT(1), B1, H2, W2, LAY(), DT(1), S],
    "qpwc_conv3x3_mish_fwd": [*CONV, B1, H2, W2, N(16, 8, 24, 512), N(1, 9), N(1, 9), S],
    "qpwc_conv3x3_mish_x3_fwd": [*CONV, B1, H2, W2, N(16, 8, 24, 512), N(1, 9), N(1, 9), S],
    "qpwc_split_bf16x3_fwd": [IN(0), OUT(1), N(8, (1 << 40) + 1), S],
    "qpwc_conv3x3_mish_f16_fwd": [*CONV, B1, H2, W2, N(16, 8, 24, 512), N(1, 9), N(1, 9), S],
    "qpwc_first_conv_mish_fwd": [*CONV, B1, N(2, 3), N(2, 3), LAY(), S],
    "qpwc_first_conv_mish_f16_fwd": [*CONV, B1, N(2, 3), N(2, 3), LAY(), S],
    "qpwc_conv3x3s2_mish_fwd": [*CONV, B1, N(2, 3), N(2, 3), S],
    "qpwc_conv3x3s2_mish_c_fwd": [*CONV, B1, N(2, 3), N(2, 3), N(32, 8, 16, 24, 256), S],
    "qpwc_conv3x3s2_mish_x3_fwd": [*CONV, B1, N(2, 3), N(2, 3), N(32, 8, 16, 24, 256), S],
    "qpwc_conv3x3s2_mish_f16_fwd": [*CONV, B1, N(2, 3), N(2, 3), N(32, 8, 16, 24, 256), S],
    "qpwc_conv3x3_same_fwd": [*CONV, B1, N(2, BIG), W2, N(3, 4, 16, 512), N(16, 8, 24, 512), N(1, 2, 3), N(0, 1, 2),
                              S],
    "qpwc_conv3x3_same_bwd_workspace_floats": [B1, N(2, BIG), W2, N(3, 4, 16, 512), N(16, 8, 24, 512), N(1, 2, 3)],
    "qpwc_conv3x3_same_bwd": [IN(0), IN(1), IN(2), IN(3), OUT(4), OUT(5), OUT(6), OUT(7), B1, N(2, BIG), W2,
                              N(3, 4, 16, 512), N(16, 8, 24, 512), N(1, 2, 3), N(0, 1, 2), S],
    "qpwc_upconv4x4s2_mish_fwd": [*CONV, B1, H2, W2, N(64, 32, 96, 512), N(16, 8, 24),
                                  N(16, 8, 18, (1 << 20) + 4, tag="stride"), S],
    "qpwc_upconv4x4s2_mish_x3_fwd": [*CONV, B1, H2, W2, N(64, 32, 96, 512), N(16, 8, 24),
                                     N(16, 8, 18, (1 << 20) + 4, tag="stride"), S],
    "qpwc_upconv4x4s2_mish_f16_fwd": [*CONV, B1, H2, W2, N(64, 32, 96, 512), N(16, 8, 24),
                                      N(16, 8, 18, (1 << 20) + 4, tag="stride"), S],
    "qpwc_upconv4x4s2_mish_cat_fwd": [IN(0), IN(1), IN(2), IN(3), N(256, 128, 258, tag="stride"),
                                      N(64, 48, 66, tag="stride"), N(16, 8, 18, tag="stride"), OUT(4), B1, H2, W2,
                                      N(64, 32, 96, 512), N(16, 8, 24), N(32, 16, 34, (1 << 20) + 4, tag="stride"), S],
    "qpwc_upconv4x4s2_mish_cat_f16_fwd": [IN(0), IN(1), IN(2), IN(3), N(256, 128, 258, tag="stride"),
                                          N(64, 48, 66, tag="stride"), N(16, 8, 18, tag="stride"), OUT(4), B1, H2, W2,
                                          N(64, 32, 96, 512), N(16, 8, 24),
                                          N(32, 16, 34, (1 << 20) + 4, tag="stride"), S],
    "qpwc_upconv4x4s2_bwd_workspace_floats": [B1, N(2, BIG), W2, N(64, 32, 96, 512), N(16, 8, 24, 256)],
    "qpwc_upconv4x4s2_bwd": [IN(0), IN(1), IN(2), IN(3), N(16, 8, 18, (1 << 24) + 4, tag="stride"), OUT(4), OUT(5),
                             OUT(6), OUT(7), B1, N(2, BIG), W2, N(64, 32, 96, 512), N(16, 8, 24, 256), N(0, 1, 2), S],
    "qpwc_image_head_fwd": [IN(0), IN(1), IN(2), OUT(3), N(4, (1 << 40) + 1), S],
    "qpwc_image_head_bwd_workspace_floats": [N(4, (1 << 40) + 1)],
    "qpwc_image_head_bwd": [IN(0), IN(1), IN(2), OUT(3), OUT(4), OUT(5), OUT(6), N(4, (1 << 40) + 1), S],
    "qpwc_upsample2x_image_fwd": [IN(0), OUT(1), B1, N(2, (1 << 29) + 1), W2, N(4, 5, 2, 3), R(1.0), S],
    "qpwc_upsample2x_image_bwd": [IN(0), OUT(1), B1, N(2, (1 << 29) + 1), W2, N(4, 5, 2, 3), R(1.0), S],
    "qpwc_avgpool_pyramid_fwd": [IN(0), OUT(1), B1, N(2, 3, BIG), W2, N(2, 5), N(1, 7, 2), S],
}

# no arguments to validate, or (qpwc_clock_probe) a kernel of the boundary file itself
EXEMPT = ("qpwc_version", "qpwc_last_error", "qpwc_strerror", "qpwc_build_info", "qpwc_flow_head_param_floats",
          "qpwc_epe_workspace_floats", "qpwc_epe_multi_workspace_floats", "qpwc_clock_probe")


def base_args(items):
    return [list(v) if isinstance(v, list) else v for _, v, _, _ in items]


def single_mutations(items):
    """[(tag, argument index, new value)]: every mutation of one argument of the base tuple."""
    base = base_args(items)
    # every buffer of the call in argument order: (argument, element of its array or None, is an output, offset)
    buffers = []
    for i, (kind, v, _, _) in enumerate(items):
        if kind in ("in", "out"):
            buffers.append((i, None, kind == "out", v))
        elif kind in ("ins", "outs"):
            buffers += [(i, k, kind == "outs", e) for k, e in enumerate(v)]

    def moved(i, k, v):
        if k is None:
            return v
        a = list(base[i])
        a[k] = v
        return a

    out = []
    for n, (i, k, is_out, off) in enumerate(buffers):
        out.append(("null", i, moved(i, k, None)))
        if k == 0:
            out.append(("null", i, None))
        out += [("align", i, moved(i, k, off + d)) for d in (2, 4, 8)]
        if is_out:
            # onto every input and every earlier output
            out += [("alias", i, moved(i, k, o2)) for n2, (_, _, out2, o2) in enumerate(buffers) if not out2 or n2 < n]
    for i, (kind, v, bad, tag) in enumerate(items):
        if kind == "n":
            out += [(tag, i, b) for b in bad]
        elif kind == "ns":
            out.append(("null", i, None))
            out += [(tag, i, moved(i, k, b)) for k in range(len(v)) for b in bad if b != v[k]]
    return out


def cases(items):
    """The base tuple, every single mutation, and one pair for every two arguments and every two different tags: the
    first mutation of each (argument, tag).  A pair holds which of two checks answers first.  Of the plain pointers
    only the first takes part with its null (the null checks of an entry point come first and together; those of
    the elements of an array do not, and all of them take part): it keeps the golden under its size limit."""
    singles = single_mutations(items)
    firsts, plain_null = {}, False
    for tag, i, v in singles:
        if tag == "null" and items[i][0] in ("in", "out"):
            if plain_null:
                continue
            plain_null = True
        firsts.setdefault((i, tag), v)
    out = [[]] + [[i, v] for _, i, v in singles]
    for ((i, ti), vi), ((j, tj), vj) in itertools.combinations(firsts.items(), 2):
        if i != j and ti != tj:
            out.append([i, vi, j, vj])
    return out


def apply(base, diff):
    args = list(base)
    for k in range(0, len(diff), 2):
        args[diff[k]] = diff[k + 1]
    return args


# ---- running a case ------------------------------------------------------------------------------------------------

class Runner:
    def __init__(self):
        self.lib = _hip.lib()
        self.buf = ctypes.create_string_buffer(N_SLOTS * SLOT + 16)
        addr = ctypes.addressof(self.buf)
        self.base = addr + (-addr) % 16

    def _ptr(self, off):
        return None if off is None else self.base + off

    def _array(self, ctype, values, convert=lambda v: v):
        if values is None:
            return None
        # room for the largest count any entry point reads (8 levels), so that a mutated count reads zeros
        return (ctype * max(len(values), 8))(*[convert(v) for v in values])

    def run(self, name, args):
        """(returned value, qpwc_last_error() afterwards).  The error text is thread-local and sticky, so a call
        that sets none would show its predecessor's: a failing call with a known text goes first."""
        restype, argtypes = _hip.PROTOTYPES[name]
        assert len(args) == len(argtypes), name
        c_args = []
        for t, v in zip(argtypes, args):
            if t is ctypes.c_void_p:
                c_args.append(self._ptr(v))
            elif t is _PVP:
                c_args.append(self._array(ctypes.c_void_p, v, self._ptr))
            elif t is _PI:
                c_args.append(self._array(ctypes.c_int, v))
            elif t is _PI64:
                c_args.append(self._array(ctypes.c_int64, v))
            else:
                c_args.append(v)
        assert self.lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL
        ret = getattr(self.lib, name)(*c_args)
        if restype is ctypes.c_char_p:
            ret = ret.decode()
        return ret, self.lib.qpwc_last_error().decode()


def write_golden(path=GOLDEN):
    if not os.environ.get("QPWC_HIP_LIB"):
        raise SystemExit("set QPWC_HIP_LIB to a library built from the parent commit: the golden is never written "
                         "from the code under test")
    runner = Runner()
    texts, functions = [], {}
    for name, items in ENTRIES.items():
        base = base_args(items)
        rows = []
        for diff in cases(items):
            ret, text = runner.run(name, apply(base, diff))
            if text not in texts:
                texts.append(text)
            rows.append([diff, ret, texts.index(text)])
        functions[name] = {"base": base, "cases": rows}
    with open(path, "w") as f:
        f.write('{"about": "function -> base arguments (pointers: offsets into one 16-byte aligned host buffer) and '
                'cases [sparse change of the base as index, value pairs; returned value; index into texts of '
                'qpwc_last_error() afterwards]; written by tests/test_capi_contract_cpu.py from ' +
                json.dumps(_hip.build_info()["build"])[1:-1] + '",\n')
        f.write('"texts": ' + json.dumps(texts, indent=0) + ',\n"functions": {\n')
        f.write(",\n".join('{}: {{"base": {}, "cases": [\n{}]}}'.format(
            json.dumps(n), json.dumps(d["base"], separators=(",", ":")),
            ",\n".join(json.dumps(r, separators=(",", ":")) for r in d["cases"])) for n, d in functions.items()))
        f.write("\n}}\n")
    print("{}: {} cases of {} functions, {} texts, {} bytes".format(
        path, sum(len(d["cases"]) for d in functions.values()), len(functions), len(texts), os.path.getsize(path)))


# ---- the tests -----------------------------------------------------------------------------------------------------

def _gpu_present():
    import torch
    return torch.cuda.is_available()


if __name__ != "__main__" and _gpu_present():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runner(hip_lib):
    return Runner()


def test_every_symbol_is_covered_or_exempt():
    assert not set(ENTRIES) & set(EXEMPT)
    assert sorted(list(ENTRIES) + list(EXEMPT)) == sorted(_hip.SYMBOLS)


def test_golden_holds_the_case_table(golden):
    """The golden was written from this table: same functions, same base tuples, same mutations in the same order."""
    assert list(golden["functions"]) == list(ENTRIES)
    for name, items in ENTRIES.items():
        rec = golden["functions"][name]
        assert rec["base"] == base_args(items), name
        assert [c[0] for c in rec["cases"]] == cases(items), name


def test_every_base_tuple_passes_validation(golden):
    """Without a device a valid call fails at its launch and nowhere earlier; a query answers."""
    for name, rec in golden["functions"].items():
        diff, ret, ti = rec["cases"][0]
        assert diff == []
        restype = _hip.PROTOTYPES[name][0]
        if restype is ctypes.c_char_p:
            assert ret != "", name
        elif restype is ctypes.c_int64:
            assert ret >= 0, name
        else:
            assert ret == _hip.E_LAUNCH and "no ROCm-capable device" in golden["texts"][ti], name


@pytest.mark.parametrize("name", list(ENTRIES))
def test_replay(name, golden, runner):
    rec = golden["functions"][name]
    differing = []
    for diff, ret, ti in rec["cases"]:
        got = runner.run(name, apply(rec["base"], diff))
        if got != (ret, golden["texts"][ti]):
            differing.append((diff, got, (ret, golden["texts"][ti])))
    assert not differing, "{} of {} cases differ; first: change {} gives {}, golden {}".format(
        len(differing), len(rec["cases"]), *differing[0])


if __name__ == "__main__":
    write_golden()
