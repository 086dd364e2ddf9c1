"""GPU suite of flow_to_image and the trainer's flow panels (qpwcnet_amd.vis on qpwc_flow_to_image_fwd).

Oracle: ``ref_flow_to_image`` / ``ref_nearest`` / ``ref_uint8``, the float64 restatement in tests/test_vis_cpu.py (the
fp32 torch composition meets the same bound there).  Bound: 1e-4, the project's kernel bound; every value is in [0, 1]
and the chain is an atan2f, a square root, a division and a handful of sums, a few 1e-7 in fp32.

LEVELS, one call: three flows of different sizes, B = 2.  Level 0 (33 x 70 = 2310 pixels) has more source pixels than
one max-tile (_hip.VIS_MAX_TILE) and no multiple of it, its largest vector in the last, partial tile of image 0 and
in the first tile of image 1; level 1 (5 x 7) is smaller than a wave; level 2 (15 x 25) is odd in both extents.
Pictures: the flows' own sizes and (37, 70) take the <scalar> stores (2310, 35, 375 and 2590 pixels: no multiple of 4),
(64, 128) takes <vec4> with 8 colour tiles (_hip.VIS_TILE) per image and (36, 70) takes it with two whole tiles and one
of 472 pixels (2520 = 2 * 1024 + 472, a multiple of 4: the partial tile of either layout, fp32 and uint8); the resized
forms have non-integer ratios without ties (ref_nearest_index asserts it).  Measured on an MI355X: see the docstrings
of the tests."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vis_cpu import (BOUND, FORMATS, random_flow, ref_flow_to_image, ref_nearest, ref_nearest_index,  # noqa: E402
                          ref_uint8, to_layout)

from qpwcnet_amd import _hip, layers, ops, synth, vis  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
B = 2
SHAPES = [(33, 70), (5, 7), (15, 25)]
SIZES = {"native": None, "scalar": (37, 70), "vec4": (64, 128), "vec4_tail": (36, 70)}
U8_SEED = 20                      # N(0, 3^2) flows: the share of elements near a uint8 step is asserted below


def make_levels(seed=0):
    """Channels-last float32 flows of SHAPES; the largest vector of level 0 sits at its last pixel in image 0 (the
    partial max-tile) and at pixel 3 in image 1 (the first max-tile), far above the N(0, 3^2) rest."""
    flows = [random_flow(seed + i, (B,) + s) for i, s in enumerate(SHAPES)]
    tile, px = _hip.VIS_MAX_TILE, SHAPES[0][0] * SHAPES[0][1]
    assert tile < px < 2 * tile and px % tile and px - 1 >= tile > 3, "level 0 no longer straddles a max-tile"
    assert float(np.abs(flows[0]).max()) < 20.0
    flows[0][0, -1, -1] = (30.0, -40.0)
    flows[0][1, 0, 3] = (-21.0, 20.0)
    return flows


LEVELS = make_levels()
LEVELS_F16 = [f.astype(np.float16) for f in LEVELS]
_REF = {}


def reference(key, flows, size):
    """float64 channels-last pictures of `flows` at `size`, computed once per key and left unchanged."""
    if (key, size) not in _REF:
        imgs = [ref_flow_to_image(f) for f in flows]
        _REF[key, size] = [i if size is None else ref_nearest(i, size) for i in imgs]
        for r in _REF[key, size]:
            r.setflags(write=False)
    return _REF[key, size]


def run(flows, size, in_format, out_format, dtype):
    ts = [dev(to_layout(f, "channels_last", in_format)) for f in flows]
    outs = ops.flow_to_image(ts, None if size is None else [size] * len(ts), in_format, dtype, out_format)
    return outs, [to_layout(o.cpu().numpy(), out_format, "channels_last") for o in outs]


def picture_sizes(size):
    return SHAPES if size is None else [size] * len(SHAPES)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("form", list(SIZES))
@pytest.mark.parametrize("out_format", FORMATS)
@pytest.mark.parametrize("in_format", FORMATS)
def test_kernels_match_the_float64_restatement(in_format, out_format, form, half):
    """Every element of the three pictures.  Measured on an MI355X: max |err| 4.8e-7 (fp32 flows) and 5.1e-7 (fp16)
    over the 32 cases; the torch composition on the CPU is at 4.6e-7."""
    size = SIZES[form]
    flows = LEVELS_F16 if half else LEVELS
    outs, got = run(flows, size, in_format, out_format, torch.float32)
    want = reference("f16" if half else "f32", [f.astype(np.float32) for f in flows], size)
    name = ops.flow_to_image_kernel(B, picture_sizes(size), torch.float32, out_format, outs)
    assert name == "flow_to_image_kernel<{}>".format("vec4" if form.startswith("vec4") else "scalar")
    for l, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape and g.dtype == np.float32 and np.isfinite(g).all()
        e = float(np.abs(g - r).max())                          # over EVERY element
        print("vis {}->{} {} {} level {}: max |err| {:.3e}".format(in_format, out_format, form,
                                                                   "f16" if half else "f32", l, e))
        assert e <= BOUND
    if size is None:
        # level 0 is normalised by the planted maxima (image 0's sits in the partial max-tile): fully saturated there
        assert got[0][0, -1, -1].min() < 1e-6 and got[0][1, 0, 3].min() < 1e-6


def test_negative_control():
    """The comparison tells a dropped tail of level 0 apart: without image 0's last pixel its maximum is several times
    smaller, and every other pixel of the image several times more saturated."""
    cut = [f.copy() for f in LEVELS]
    cut[0][0, -1, -1] = 0.0
    _, got = run(LEVELS, None, "channels_last", "channels_last", torch.float32)
    assert float(np.abs(got[0][0, :-1] - ref_flow_to_image(cut[0])[0, :-1]).max()) > 1000 * BOUND
    assert float(np.abs(got[0][1] - ref_flow_to_image(cut[0])[1]).max()) <= BOUND          # image 1 keeps its own


@pytest.mark.parametrize("form", list(SIZES))
@pytest.mark.parametrize("out_format", FORMATS)
@pytest.mark.parametrize("in_format", FORMATS)
def test_uint8_pictures(in_format, out_format, form):
    """uint8 against float64: at most one level off, and only where the float64 value times 255.5 lies within 1e-3 of a
    whole number; those elements may be at most 1 % (0.15 % of these pictures at the flows' own sizes, 0.41 % to
    0.44 % resized: a property of the restatement; on an MI355X no element is off anywhere else)."""
    size = SIZES[form]
    flows = [random_flow(U8_SEED + i, (B,) + s) for i, s in enumerate(SHAPES)]
    outs, got = run(flows, size, in_format, out_format, torch.uint8)
    want = reference("u8", flows, size)
    name = ops.flow_to_image_kernel(B, picture_sizes(size), torch.uint8, out_format, outs)
    assert name == "flow_to_image_kernel<{}>".format("vec4" if form.startswith("vec4") else "scalar")
    near = total = 0
    for g, r in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == r.shape
        x = r * 255.5
        close = np.abs(x - np.rint(x)) < 1e-3
        diff = np.abs(g.astype(np.int64) - ref_uint8(r).astype(np.int64))
        assert diff.max() <= 1 and not diff[~close].any()
        near, total = near + int(close.sum()), total + close.size
    print("vis uint8 {}->{} {}: {:.3f} % of the elements near a step".format(in_format, out_format, form,
                                                                           100.0 * near / total))
    assert near <= 0.01 * total


def test_eight_levels_in_one_call_native_vec4():
    """The most levels a call takes, fp32 and fp16 mixed, every picture at its flow's own size with a multiple of 4
    pixels: <vec4> with partial colour tiles (40 x 52 = 2080 = 2 * 1024 + 32) and partial max-tiles (2080 = 2048 + 32)."""
    shapes = [(2, 2), (2, 4), (4, 8), (8, 16), (16, 32), (40, 52), (6, 6), (12, 3)]
    assert shapes[5][0] * shapes[5][1] % _hip.VIS_TILE == 32 and shapes[5][0] * shapes[5][1] % _hip.VIS_MAX_TILE == 32
    flows = [random_flow(40 + i, (B,) + s) for i, s in enumerate(shapes)]
    ts = [dev(f).half() if i % 2 else dev(f) for i, f in enumerate(flows)]
    for out_format in FORMATS:
        for dtype in (torch.float32, torch.uint8):
            outs = ops.flow_to_image(ts, None, "channels_last", dtype, out_format)
            assert ops.flow_to_image_kernel(B, shapes, dtype, out_format, outs) == "flow_to_image_kernel<vec4>"
            for o, t in zip(outs, ts):
                r = ref_flow_to_image(t.float().cpu().numpy())
                g = to_layout(o.cpu().numpy(), out_format, "channels_last")
                if dtype == torch.float32:
                    assert float(np.abs(g - r).max()) <= BOUND
                else:
                    x = r * 255.5
                    diff = np.abs(g.astype(np.int64) - ref_uint8(r).astype(np.int64))
                    assert diff.max() <= 1 and not diff[np.abs(x - np.rint(x)) >= 1e-3].any()
    with pytest.raises(ValueError, match="1..8"):
        ops.flow_to_image(ts + ts[:1])


@pytest.mark.parametrize("data_format", FORMATS)
def test_all_zero_image_beside_a_moving_one(data_format):
    flow = random_flow(7, (B, 9, 11))
    flow[0] = 0.0
    img = vis.flow_to_image(dev(to_layout(flow, "channels_last", data_format)), data_format)
    img = to_layout(img.cpu().numpy(), data_format, "channels_last")
    assert np.isfinite(img).all() and (img[0] == 1.0).all()
    assert float(np.abs(img[1] - ref_flow_to_image(flow)[1]).max()) <= BOUND and img[1].min() < 0.5
    panel = vis.flow_panels([dev(to_layout(flow, "channels_last", data_format))], data_format=data_format)[0]
    assert panel.dtype == torch.uint8 and bool((panel[0] == 255).all())
    one = vis.flow_to_image(dev(to_layout(flow, "channels_last", data_format))[1], data_format)       # rank 3
    assert np.array_equal(to_layout(one[None].cpu().numpy(), data_format, "channels_last")[0], img[1])


def test_two_calls_are_bitwise_equal():
    ts = [dev(f) for f in LEVELS]
    for dtype in (torch.float32, torch.uint8):
        for size in (None, (64, 128)):
            a = ops.flow_to_image(ts, None if size is None else [size] * 3, "channels_last", dtype, "channels_last")
            b = ops.flow_to_image(ts, None if size is None else [size] * 3, "channels_last", dtype, "channels_last")
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the picture does not depend on the layouts or on the store form either
    a = ops.flow_to_image(ts[2:], [(20, 25)], "channels_last", torch.float32, "channels_last")[0]       # vec4
    b = ops.flow_to_image([ts[2].permute(0, 3, 1, 2).contiguous()], [(20, 25)], "channels_first", torch.float32,
                          "channels_first")[0]
    assert torch.equal(a, b.permute(0, 2, 3, 1))
    c = ops.flow_to_image(ts[1:], [(20, 25), (20, 25)], "channels_last", torch.float32, "channels_last")   # both vec4
    d = ops.flow_to_image(ts[1:], [(5, 7), (20, 25)], "channels_last", torch.float32, "channels_last")     # scalar
    assert torch.equal(c[1], d[1]) and torch.equal(c[1], a)


def test_graph_replay_follows_the_flows():
    """Captured once on one stream, replayed after the flows changed in place: the pictures follow the new maxima, so no
    value went through the host and the workspace carries nothing from one run to the next."""
    first = [f.copy() for f in LEVELS]
    second = [random_flow(60 + i, (B,) + s, scale=0.5) for i, s in enumerate(SHAPES)]
    second[0][1, 20, 5] = (0.0, 9.0)
    ts = [dev(f) for f in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.flow_to_image(ts, [(64, 128)] * 3, "channels_last", torch.float32, "channels_first")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.flow_to_image(ts, [(64, 128)] * 3, "channels_last", torch.float32, "channels_first")
    for values in (first, second, second, first):
        for t, v in zip(ts, values):
            t.copy_(dev(v))
        graph.replay()
        torch.cuda.synchronize()
        for o, v in zip(outs, values):
            want = ref_nearest(ref_flow_to_image(v), (64, 128))
            assert float(np.abs(to_layout(o.cpu().numpy(), "channels_first", "channels_last") - want).max()) <= BOUND
    graph.replay()                                              # `first` again: bit for bit what eager gives
    torch.cuda.synchronize()
    eager = ops.flow_to_image(ts, [(64, 128)] * 3, "channels_last", torch.float32, "channels_first")
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))


def test_flow_panels_of_the_model():
    """ShowImageCallback.on_batch_end's pictures for [label] + list(FlowerModel(ims)) at 64 x 64, the smallest input
    whose coarsest level (2 x 2) the warps take: the label and the model's six flows (five estimates and the final
    upsampled one) in one call, equal to the per-level path."""
    hw = (64, 64)
    net = layers.FlowerModel(data_format="channels_last")
    net.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_weights(42, hw).items()})
    net = net.to(DEV).eval()
    pairs, label = synth.make_frames(B, hw[0], hw[1], seed=5)
    pairs, label = dev(pairs), dev(label)
    with torch.no_grad():
        flows = [label] + list(net(pairs))
    assert [tuple(f.shape[1:3]) for f in flows] == [hw, (2, 2), (4, 4), (8, 8), (16, 16), (32, 32), hw]
    panels = vis.flow_panels(flows)
    assert len(panels) == len(flows) == 7
    for p, f in zip(panels, flows):
        assert p.dtype == torch.uint8 and tuple(p.shape) == (B,) + hw + (3,) and p.is_contiguous()
        img = vis.flow_to_image(f)
        iy, ix = (dev(ref_nearest_index(n, m)) for n, m in zip(hw, f.shape[1:3]))
        assert torch.equal(p, vis.to_uint8(img[:, iy][:, :, ix]))
        assert float(p.float().std()) > 1.0                                     # a picture, not a flat field
    floats = vis.flow_panels(flows, dtype=torch.float32)
    assert all(torch.equal(vis.to_uint8(a), b) for a, b in zip(floats, panels))
    cf = vis.flow_panels([f.permute(0, 3, 1, 2).contiguous() for f in flows], data_format="channels_first")
    assert all(torch.equal(a, b) for a, b in zip(cf, panels))
    small = vis.flow_panels(flows[1:4], size=(8, 8))
    assert all(tuple(p.shape) == (B, 8, 8, 3) for p in small)
