"""The shapes of tests/test_gpu_eval_scale.py, and the proof without a GPU that each still reaches the device code it is
chosen for: the flow metrics (csrc/flow_quality.hip) where the fold kernel's two loops iterate, and the masked flow losses
(csrc/masked_loss.hip on the bodies of csrc/loss_common.h) in the forms that tests/test_gpu_masked_loss.py does not reach
-- the scalar backward, sum plans with unequal steps, and second trips of the pixel walk.

The grid constants are read from the kernel sources, so a raised constant that turns a case back into a one-trip case
fails here; the kernel selection is the library's own host query (ops.masked_loss_kernel / ops.flow_quality_kernel).  The
float64 oracles run here over the very inputs the GPU module uses: ``ref_flow_quality`` / ``ref_sums`` of
tests/test_flow_quality_cpu.py, and ``loss.multiscale_masked_torch`` for the losses.  Three mutated restatements of the
fold kernel -- chunks from 64 on dropped, images from 32 on dropped from the state, stale rows in the partial round --
must each miss the bounds on these inputs (test_the_comparison_sees_the_planted_fold_defects).

Measured on the CPU: the fp32 torch composition of the flow metrics stays within 4.9e-7 px (EPE-type means), 1.1e-6
degrees (aae) and 0.5 ulp (count ratios) of float64 on the three fold cases; the fp32 torch chain of the masked losses
within 0.014 of the 1e-5 bound on every row."""
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_quality_cpu import (CHUNK, CHUNKS, FIELDS, LAST, channels_last, check, check_state,  # noqa: E402
                                   make_flows, masks, near_a_threshold, ref_flow_quality, ref_scores, ref_sums, tensor,
                                   violations)
from test_masked_loss_cpu import CODES, KINDS, make_loss, ref_valid  # noqa: E402

from qpwcnet_amd import loss, metrics  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")


def _constants(name, *keys):
    text = open(os.path.join(CSRC, name)).read()
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*(\d+)\s*;".format(k), text)
        assert len(m) == 1, (name, k, m)
        out[k] = int(m[0])
    return out


FQ = _constants("flow_quality.hip", "kFlowQualFoldThreads", "kFlowQualChunk")
ML = _constants("masked_loss.hip", "kLossThreads", "kLossPixBlocks", "kLossTileBlocks", "kLossTile", "kLossBwdBlocks")
MAX_STEPS = _constants("loss_common.h", "kLossMaxSteps")["kLossMaxSteps"]
WAVES = FQ["kFlowQualFoldThreads"] // 64          # images per round of the fold kernel
LANES = 64                                        # chunks per trip of a wave


# ==== flow metrics: where the fold loops iterate =======================================================================
def shape_of(whole, extra=3):
    """(H, W) with H * W = whole * CHUNK + r, 0 < r < 64, and an odd width: `whole` whole chunks and a last one shorter
    than a wave.  r = extra, or the nearest larger value at which the pixel count has an odd factor."""
    n = whole * CHUNK + extra
    while n < whole * CHUNK + 64:
        for w in range(int(math.isqrt(n)) | 1, 2, -2):
            if n % w == 0:
                return n // w, w
        n += 1
    raise AssertionError("no shape with {} whole chunks".format(whole))


ROUNDS_B, CHUNKS_B, BOTH_B = 35, 3, 17
CHUNKS_HW, BOTH_HW = shape_of(130), shape_of(64)
TAIL = CHUNKS_HW[0] * CHUNKS_HW[1] - 2 * LANES * CHUNK      # fold_chunks: the pixels of the chunks from 128 on
BOTH_LAST = BOTH_HW[0] * BOTH_HW[1] - 64 * CHUNK            # fold_both: the pixels of chunk 64


def _sigmas(batch):
    """An error level of its own for every image: 0.3 px (even) / 4 px (odd), growing by 5 % per image."""
    return tuple((0.3 if n % 2 == 0 else 4.0) * (1.0 + 0.05 * n) for n in range(batch))


def _fold_chunks_flows():
    """make_flows on CHUNKS_HW with image 1 slower than 40 px in chunks 0..127 (a faster pixel is halved, its error
    kept) and at (50, 30), 58 px, in every pixel of the chunks from 128 on."""
    truth, pred = make_flows(42, CHUNKS_HW, sigmas=(0.3, 4.0, 1.0), batch=CHUNKS_B)
    n = CHUNKS_HW[0] * CHUNKS_HW[1]
    ft, fp = truth.reshape(CHUNKS_B, n, 2), pred.reshape(CHUNKS_B, n, 2)
    err = fp[1] - ft[1]
    fast = np.hypot(ft[1, :, 0], ft[1, :, 1]) >= 37.0
    ft[1, fast] *= np.float32(0.5)
    ft[1, -TAIL:] = np.float32([50.0, 30.0])
    fp[1] = ft[1] + err
    return truth, pred


def away_from_thresholds_fast(truth, pred, dtype):
    """test_flow_quality_cpu.away_from_thresholds -- every pixel within MARGIN of a threshold moved by 0.01 px at a time,
    nothing left out -- with the rounds after the first confined to the offending pixels: these cases have millions."""
    truth, shadow = truth.copy(), pred.astype(np.float32).copy()
    out = shadow.astype(dtype)
    idx = np.nonzero(near_a_threshold(truth, out))
    for _ in range(400):
        if idx[0].size == 0:
            return truth, out
        t, s = truth[idx], shadow[idx]                                    # (k, 2) copies
        as_image = lambda a: a.reshape(-1, 1, 1, 2)
        near = near_a_threshold(as_image(t), as_image(s.astype(dtype))).reshape(-1)
        speed = near_a_threshold(as_image(t), as_image(s.astype(dtype)), which="speed").reshape(-1)
        t[speed, 0] += np.float32(0.01)
        s[near, 0] += np.float32(0.01)
        truth[idx], shadow[idx], out[idx] = t, s, s.astype(dtype)
        idx = tuple(i[near] for i in idx)
    raise AssertionError("could not move every pixel away from the thresholds")


def _flow_case(truth, pred, valid, occluded, data_format="channels_last", half=False):
    truth, pred = away_from_thresholds_fast(truth, pred, np.float16 if half else np.float32)
    if data_format == "channels_first":
        truth, pred = (np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))) for a in (truth, pred))
    c = dict(truth=truth, pred=pred, data_format=data_format, valid=valid, occluded=occluded)
    for k in ("truth", "pred", "valid", "occluded"):
        c[k].setflags(write=False)
    return c


FLOW_NAMES = ("fold_rounds", "fold_chunks", "fold_both")


@functools.lru_cache(maxsize=None)
def flow_case(name):
    """dict(truth, pred, data_format, valid, occluded) of read-only numpy arrays, as test_flow_quality_cpu.CASES holds
    them; built from seeds on first use."""
    if name == "fold_rounds":
        v, o = masks(41, CHUNKS, batch=ROUNDS_B)
        return _flow_case(*make_flows(40, CHUNKS, sigmas=_sigmas(ROUNDS_B), batch=ROUNDS_B), v, o)
    if name == "fold_chunks":
        v, o = masks(43, CHUNKS_HW, batch=CHUNKS_B, last=TAIL)
        return _flow_case(*_fold_chunks_flows(), v, o)
    assert name == "fold_both"
    v, o = masks(45, BOTH_HW, batch=BOTH_B, last=BOTH_LAST)
    return _flow_case(*make_flows(44, BOTH_HW, sigmas=_sigmas(BOTH_B), batch=BOTH_B), v, o,
                      data_format="channels_first", half=True)


_REF = {}


def flow_geometry(name):
    """(B, H, W, chunks) of a flow case."""
    c = flow_case(name)
    t, _ = channels_last(c)
    Bn, H, W, _ = t.shape
    return Bn, H, W, -(-(H * W) // CHUNK)


def flow_reference(name):
    """(ref_flow_quality, ref_sums [B, 15]) of a flow case in float64, computed once and left unchanged."""
    if name not in _REF:
        c = flow_case(name)
        t, p = channels_last(c)
        sums = ref_sums(t, p, c["valid"], c["occluded"])
        scores = ref_scores(sums, t.shape[1] * t.shape[2])
        sums.setflags(write=False)
        for a in scores.values():
            a.setflags(write=False)
        _REF[name] = (scores, sums)
    return _REF[name]


def run_flow_case(name, device="cpu", images=None, state=None, **kw):
    """metrics.flow_quality on a case (or on the images of `images`, a slice) -> FlowScores."""
    c = flow_case(name)
    sl = slice(None) if images is None else images
    m = lambda a: tensor(a[sl]).to(device)
    return metrics.flow_quality(m(c["truth"]), m(c["pred"]), valid=m(c["valid"]), occluded=m(c["occluded"]),
                                data_format=c["data_format"], state=state, **kw)


def chunk_sums(name):
    """float64 [B, chunks, 15]: ref_sums of every chunk of kFlowQualChunk consecutive pixels on its own."""
    c = flow_case(name)
    t, p = channels_last(c)
    Bn, H, W, chunks = flow_geometry(name)
    ft, fp = t.reshape(Bn, 1, H * W, 2), p.reshape(Bn, 1, H * W, 2)
    fv, fo = c["valid"].reshape(Bn, 1, H * W), c["occluded"].reshape(Bn, 1, H * W)
    cut = lambda a, k: a[:, :, k * CHUNK:(k + 1) * CHUNK]
    return np.stack([ref_sums(cut(ft, k), cut(fp, k), cut(fv, k), cut(fo, k)) for k in range(chunks)], axis=1)


def fold_state(sums, pixels, defect=None):
    """flow_quality_fold_kernel's loop over rounds of WAVES images restated on float64 per-image sums [B, 15] -> the 17
    state values of one call on a zero state.  defect "two_rounds": the images from 2 WAVES on never reach the state;
    "stale": the guard `n0 + w < B` of the partial round is missing, so the rows that the round's missing waves left
    behind in the round before are added again."""
    Bn = len(sums)
    run, res = np.zeros(15), np.zeros((WAVES, 15))
    for n0 in range(0, Bn, WAVES):
        for w in range(WAVES):
            if n0 + w < Bn:
                res[w] = sums[n0 + w]
        if defect == "two_rounds" and n0 >= 2 * WAVES:
            continue
        for w in range(WAVES):
            if n0 + w < Bn or defect == "stale":
                run = run + res[w]
    return np.concatenate([run, [float(Bn), float(Bn) * pixels]])


def test_the_flow_cases_reach_the_fold_loops(hip_lib):
    from qpwcnet_amd import _hip, ops
    assert FQ["kFlowQualChunk"] == CHUNK == _hip.FLOW_QUALITY_CHUNK and FQ["kFlowQualFoldThreads"] % 64 == 0
    text = open(os.path.join(CSRC, "flow_quality.hip")).read()
    assert text.count("n0 += kFlowQualFoldThreads / 64") == 1 and text.count("t += 64") == 1     # the two loops, as read
    assert text.count("n0 + w < B") == 1
    # fold_rounds: two whole rounds and a partial third; three chunks, the last one short, an odd width
    Bn, H, W, chunks = flow_geometry("fold_rounds")
    assert Bn == ROUNDS_B > 2 * WAVES and Bn % WAVES != 0 and Bn < 3 * WAVES
    assert (H, W) == CHUNKS and chunks == 3 and W % 2 == 1 and 0 < LAST < 64
    # fold_chunks: lanes 0..63 take three trips, the last one partial; the last chunk is shorter than a wave
    Bn, H, W, chunks = flow_geometry("fold_chunks")
    assert Bn == CHUNKS_B and 2 * LANES < chunks <= 3 * LANES and chunks % LANES != 0 and W % 2 == 1
    assert 0 < H * W - (chunks - 1) * CHUNK < 64 and TAIL == H * W - 2 * LANES * CHUNK > CHUNK
    # fold_both: a second round of one wave and a second trip of one lane
    Bn, H, W, chunks = flow_geometry("fold_both")
    assert Bn == BOTH_B and WAVES < Bn < 2 * WAVES and chunks == LANES + 1 and W % 2 == 1 and 0 < BOTH_LAST < 64
    c = flow_case("fold_both")
    assert c["data_format"] == "channels_first" and c["pred"].dtype == np.float16 and c["truth"].shape == (Bn, 2, H, W)
    for name in FLOW_NAMES:
        Bn, H, W, chunks = flow_geometry(name)
        assert ops.flow_quality_kernel(Bn, H, W) == "flow_quality_tile_kernel"
        assert hip_lib.qpwc_flow_quality_workspace_floats(Bn, H, W) == Bn * chunks * 15


def test_the_flow_cases_have_their_properties():
    for name in FLOW_NAMES:
        c = flow_case(name)
        t, p = channels_last(c)
        assert not near_a_threshold(t, p, c["valid"]).any(), name              # the bounds' precondition
        assert c["valid"] is not None and c["occluded"] is not None            # both masks
        scores, sums = flow_reference(name)
        Bn = len(sums)
        # every image its own content and error level: no two images share a sum, the levels alternate
        assert len({tuple(row) for row in sums}) == Bn, name
        assert len(set(np.round(scores["epe"], 6))) == Bn, name
        assert all(scores["epe"][n + 1] > 3 * scores["epe"][n] for n in range(0, Bn - 1, 2) if name != "fold_chunks")
        assert all(np.isfinite(scores[k]).all() for k in FIELDS if k not in ("epe_s40",)), name
        for n in range(Bn):
            assert 0.05 <= 1.0 - c["valid"][n].mean() <= 0.5, (name, n)
    # fold_chunks, image 1: its only s40+ and its only occluded pixels lie in the chunks from 128 on
    c = flow_case("fold_chunks")
    t, _ = channels_last(c)
    m = np.hypot(t[1, ..., 0].astype(np.float64), t[1, ..., 1]).reshape(-1)
    assert (m[:-TAIL] < 40).all() and (m[-TAIL:] > 40).all()
    occ = c["occluded"][1].reshape(-1)
    assert occ[-TAIL:].all() and occ.sum() == TAIL and c["valid"][1].reshape(-1)[-TAIL:].all()
    per_chunk = chunk_sums("fold_chunks")
    assert not per_chunk[1, :2 * LANES, 13].any() and per_chunk[1, 2 * LANES:, 13].all()      # n of the s40+ bin
    assert not per_chunk[1, :2 * LANES, 7].any() and per_chunk[1, 2 * LANES:, 7].all()        # n occluded
    assert per_chunk[0, :, 13].any() and per_chunk[2, :2 * LANES, 7].all()


@pytest.mark.parametrize("name", list(FLOW_NAMES))
def test_flow_torch_path_against_the_restatement(name):
    """The fp32 torch composition on the CPU within the kernels' bounds of float64.  Measured: at most 4.9e-7 px in the
    EPE-type means (fold_rounds), 1.1e-6 degrees in aae (fold_rounds), count ratios 0.5 ulp."""
    scores, sums = flow_reference(name)
    c = flow_case(name)
    assert all(np.array_equal(np.isnan(scores[k]), np.isnan(ref_flow_quality(
        c["truth"], c["pred"], c["valid"], c["occluded"], data_format=c["data_format"])[k])) for k in FIELDS)
    check("torch " + name, run_flow_case(name), scores)
    per_chunk = chunk_sums(name)
    whole = per_chunk.sum(axis=1)
    assert np.array_equal(whole[:, [0, 3, 4, 5, 6, 7, 9, 11, 13]], sums[:, [0, 3, 4, 5, 6, 7, 9, 11, 13]])
    assert np.abs(whole - sums).max() <= 1e-9 * np.abs(sums).max()


def test_flow_state_on_the_cpu_is_the_restated_fold():
    """fold_rounds twice into one FlowQuality on the CPU: check_state against float64, and the state of fold_state's
    restatement of the kernel's loop over rounds passes the same check."""
    scores, sums = flow_reference("fold_rounds")
    pixels = CHUNKS[0] * CHUNKS[1]
    m = metrics.FlowQuality(data_format="channels_last")
    c = flow_case("fold_rounds")
    args = [tensor(c[k]) for k in ("truth", "pred", "valid", "occluded")]
    per = [m.update_state(args[0], args[1], valid=args[2], occluded=args[3]) for _ in range(2)]
    check_state(m, per, np.concatenate([sums, sums]), pixels, images=2 * ROUNDS_B)
    fake = metrics.FlowQuality(data_format="channels_last")
    fake.state = torch.from_numpy(fold_state(sums, pixels))
    check_state(fake, per[:1], sums, pixels, images=ROUNDS_B)


def test_the_comparison_sees_the_planted_fold_defects():
    """Three defects the B = 2, three-chunk cases cannot show, restated on the float64 sums of these inputs: each must
    miss check / check_state."""
    # a wave that sums only its first trip: every image's chunks from 64 on are dropped
    for name in ("fold_chunks", "fold_both"):
        scores, sums = flow_reference(name)
        Bn, H, W, chunks = flow_geometry(name)
        per_chunk = chunk_sums(name)
        assert violations(ref_scores(per_chunk.sum(axis=1), H * W), scores)[0] == []
        bad, err = violations(ref_scores(per_chunk[:, :LANES].sum(axis=1), H * W), scores)
        assert "valid" in bad, (name, err)
        if name == "fold_chunks":
            assert {"epe", "epe_occ", "epe_s40"} <= set(bad), bad
        # and the second trip alone dropped (chunks 64..127), as a stride of 128 would
        keep = [k for k in range(chunks) if not LANES <= k < 2 * LANES]
        bad, err = violations(ref_scores(per_chunk[:, keep].sum(axis=1), H * W), scores)
        assert "valid" in bad or name == "fold_both", (name, err)
    # the state: images from 32 on dropped; the rows of the round before added again in the partial round
    scores, sums = flow_reference("fold_rounds")
    pixels = CHUNKS[0] * CHUNKS[1]
    per = [run_flow_case("fold_rounds")]
    for defect in ("two_rounds", "stale"):
        state = fold_state(sums, pixels, defect)
        assert state[0] != sums[:, 0].sum() and state[15] == ROUNDS_B
        fake = metrics.FlowQuality(data_format="channels_last")
        fake.state = torch.from_numpy(state)
        with pytest.raises(AssertionError):
            check_state(fake, per, sums, pixels, images=ROUNDS_B)
        # the pixel-weighted result alone shows it as well
        got = ref_scores(state[:15], ROUNDS_B * pixels)
        bad, err = violations({k: np.float32(got[k]) for k in FIELDS}, ref_scores(sums.sum(axis=0), ROUNDS_B * pixels))
        assert "valid" in bad and "epe" in bad, (defect, err)
    # fold_both has its own partial round: one image in the second
    _, sums = flow_reference("fold_both")
    px = BOTH_HW[0] * BOTH_HW[1]
    assert fold_state(sums, px, "stale")[0] - sums[:, 0].sum() == sums[1:WAVES, 0].sum() > 0


# ==== masked losses: the forms no other case reaches ===================================================================
TILE_PLAN_HW = (3, 64, 128)
PLAN_FACTORS = {"eight_steps": [(2, 16), (32, 32), (1, 4), (8, 32), (2, 8)],      # unequal per axis, not in area order
                "ten_steps_x_first": [(1, 4), (1, 32), (32, 32)],
                "ten_steps_y_first": [(4, 1), (32, 1), (32, 32)]}


def _plan_row(factors):
    B, H, W = TILE_PLAN_HW
    return (B, H, W, [(H // sh, W // sw) for sh, sw in factors])


# name -> [(B, H, W, [(h, w) per level])]
MASKED = {
    # masked_loss_bwd_kernel's scalar form: n = B * h * w * 2 with n % 4 == 2; one trip, then past one trip
    "bwd_scalar": [(1, 42, 70, [(21, 35)]), (3, 402, 666, [(201, 333)])],
    # masked_loss_tile_kernel: 1x2 and 2x1 sum steps of the count plane, a 32x32 factor, kLossMaxSteps steps
    "tile_plan": [_plan_row(f) for f in PLAN_FACTORS.values()],
    # masked_loss_pixel_kernel's area walk (3 x 3) past one trip
    "pixel_loop_area": [(3, 900, 900, [(300, 300)])],
    # ... and its bilinear walk with renormalised corners, ratios 2, 2.5 and 1.875 (exact in fp32)
    "pixel_loop_bilinear": [(5, 480, 960, [(240, 480), (192, 384), (256, 512)])],
}
MASKED_KINDS = {"bwd_scalar": KINDS, "tile_plan": ("v2",), "pixel_loop_area": ("v2",), "pixel_loop_bilinear": ("mse",)}
MASKED_KERNEL = {"bwd_scalar": "masked_loss_pixel_kernel", "tile_plan": "masked_loss_tile_kernel",
                 "pixel_loop_area": "masked_loss_pixel_kernel", "pixel_loop_bilinear": "masked_loss_pixel_kernel"}
MASKED_PARAMS = [(name, i, kind) for name in MASKED for i in range(len(MASKED[name])) for kind in MASKED_KINDS[name]]
# what the 32 x 32 tiles of the tile_plan ground truth hold, in tile order (image, tile row, tile column); the tiles
# behind the list are 30 % random.  "gt": the invalid pixels are NaN / 1e10 in the ground truth under a mask of ones
TILE_KINDS = (("empty", "mask"), ("corner00", "mask"), ("corner01", "gt"), ("corner10", "mask"), ("corner11", "gt"),
              ("edge", "mask"), ("full", "mask"), ("empty", "gt"), ("edge_left", "gt"))
ONE_PIXEL = {"corner00": (0, 0), "corner01": (0, 31), "corner10": (31, 0), "corner11": (31, 31), "edge": (0, 15),
             "edge_left": (16, 0)}


def tile_steps(H, W, shapes):
    """loss_tile_plan's sum steps restated: the levels in area order (stable), each reached by 2x2 / 2x1 / 1x2 steps."""
    factors = sorted(((H // h, W // w) for h, w in shapes), key=lambda f: f[0] * f[1])
    cy, cx, steps = 1, 1, []
    for ty, tx in factors:
        assert ty >= cy and tx >= cx and (ty, tx) != (cy, cx), "not nested"
        while (cy, cx) != (ty, tx):
            ry, rx = (2 if cy < ty else 1), (2 if cx < tx else 1)
            cy, cx = cy * ry, cx * rx
            steps.append((ry, rx))
    return steps


def _random_validity(gen, B, H, W, block=6):
    """About 30 % of the pixels: half of the pixels of 60 % of the block x block squares, so that level pixels without
    a valid ground-truth pixel exist beside full ones."""
    squares = torch.rand(B, -(-H // block), -(-W // block), generator=gen) < 0.6
    keep = squares.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :H, :W]
    return keep & (torch.rand(B, H, W, generator=gen) < 0.5)


def _tile_plan_validity(gen, gt):
    """-> (gt with NaN / 1e10 planted, mask): validity by 32 x 32 tile, TILE_KINDS first, 30 % random behind them."""
    B, H, W, _ = gt.shape
    T = ML["kLossTile"]
    keep = _random_validity(gen, B, H, W, block=4)
    mask = torch.ones(B, H, W, dtype=torch.bool)
    tiles = [(b, ty, tx) for b in range(B) for ty in range(H // T) for tx in range(W // T)]
    for k, (b, ty, tx) in enumerate(tiles):
        what, how = TILE_KINDS[k] if k < len(TILE_KINDS) else ("random", "mask" if k % 2 else "gt")
        win = (b, slice(ty * T, (ty + 1) * T), slice(tx * T, (tx + 1) * T))
        if what == "empty":
            keep[win] = False
        elif what == "full":
            keep[win] = True
        elif what in ONE_PIXEL:
            keep[win] = False
            keep[b, ty * T + ONE_PIXEL[what][0], tx * T + ONE_PIXEL[what][1]] = True
        if how == "mask":
            mask[win] = keep[win]
        else:
            bad = ~keep[win]
            junk = torch.where(torch.rand(T, T, generator=gen) < 0.5, float("nan"), 1e10)
            gt[win][bad] = junk[bad][:, None].expand(-1, 2)
    return gt, mask


@functools.lru_cache(maxsize=None)
def masked_inputs(name, index, kind):
    """-> (gt (B,H,W,2) float32, valid (B,H,W) bool, [pred (B,h,w,2) float32 holding fp16 values]), channels-last CPU
    tensors from a seed.  The predictions lie 0.25..0.75 or 2..6 off the level's float64 ground truth in every channel,
    random signs: no residual near 0, where the norms have a kink and sign() would amplify a rounding."""
    B, H, W, shapes = MASKED[name][index]
    gen = torch.Generator().manual_seed(1000 * sorted(MASKED).index(name) + 10 * index + KINDS.index(kind))
    gt = torch.randn(B, H, W, 2, generator=gen) * 4.0
    if name == "tile_plan":
        gt, valid = _tile_plan_validity(gen, gt)
    else:
        valid = _random_validity(gen, B, H, W)
    base = loss.masked_ground_truth_torch(make_loss(kind, "channels_last"), gt.double(), shapes, valid)[0]
    preds = []
    for g in base:
        mag = (0.25 + 0.5 * torch.rand(g.shape, generator=gen)) * torch.where(torch.rand(g.shape, generator=gen) < 0.5, 1.0, 8.0)
        sign = torch.where(torch.rand(g.shape, generator=gen) < 0.5, -1.0, 1.0)
        preds.append((g + sign * mag).half().float())
    return gt, valid, preds


@functools.lru_cache(maxsize=None)
def masked_oracle(name, index, kind, scale=1.0):
    """loss.multiscale_masked_torch in float64 over masked_inputs -> (per-level losses, counts, d (scale * sum) / d preds,
    level masks), channels-last, computed once per row."""
    gt, valid, preds = masked_inputs(name, index, kind)
    obj = make_loss(kind, "channels_last")
    xs = [p.double().requires_grad_() for p in preds]
    _, per, counts = loss.multiscale_masked_torch(obj, gt.double(), xs, valid)
    (scale * per).sum().backward()
    masks_ = loss.masked_ground_truth_torch(obj, gt.double(), MASKED[name][index][3], valid)[1]
    return per.detach(), counts, [x.grad for x in xs], masks_


def test_masked_rows_take_the_kernel_and_the_trips_they_claim(hip_lib):
    from qpwcnet_amd import _hip, ops
    assert (ML["kLossThreads"], ML["kLossPixBlocks"], ML["kLossTileBlocks"], ML["kLossTile"]) == (
        _hip.MASKED_LOSS_THREADS, _hip.MASKED_LOSS_PIX_BLOCKS, _hip.MASKED_LOSS_TILE_BLOCKS, _hip.MASKED_LOSS_TILE)
    for name, rows in MASKED.items():
        for B, H, W, shapes in rows:
            for kind in MASKED_KINDS[name]:
                assert ops.masked_loss_kernel(CODES[kind], B, H, W, shapes) == MASKED_KERNEL[name], (name, kind, shapes)
    trips = lambda work, per_trip: -(-work // per_trip)
    pixel_trip, bwd_trip = ML["kLossPixBlocks"] * ML["kLossThreads"], ML["kLossBwdBlocks"] * ML["kLossThreads"]
    # bwd_scalar: never whole float4 (the masked shell takes the scalar form on n % 4 alone); one trip, then two
    text = open(os.path.join(CSRC, "masked_loss.hip")).read()
    assert text.count("lg.n[l] % 4 == 0") == 1
    sizes = [B * h * w * 2 for B, H, W, shapes in MASKED["bwd_scalar"] for h, w in shapes]
    assert all(n % 4 == 2 for n in sizes) and trips(sizes[0], bwd_trip) == 1 and trips(sizes[1], bwd_trip) == 2
    assert sizes[1] % bwd_trip
    # tile_plan: the steps of loss_tile_plan, restated
    B, H, W = TILE_PLAN_HW
    assert H % ML["kLossTile"] == 0 and W % ML["kLossTile"] == 0 and B * (H // 32) * (W // 32) > len(TILE_KINDS) + 8
    row = dict(zip(PLAN_FACTORS, MASKED["tile_plan"]))
    steps = tile_steps(H, W, row["eight_steps"][3])
    assert len(steps) == 8 and {(1, 2), (2, 1), (2, 2)} <= set(steps)
    areas = [sh * sw for sh, sw in PLAN_FACTORS["eight_steps"]]
    assert areas != sorted(areas) and any(sh != sw for sh, sw in PLAN_FACTORS["eight_steps"]) and max(areas) == 1024
    x_first, y_first = (tile_steps(H, W, row[k][3]) for k in ("ten_steps_x_first", "ten_steps_y_first"))
    assert len(x_first) == len(y_first) == MAX_STEPS == 10
    assert x_first == [(1, 2)] * 5 + [(2, 1)] * 5 and y_first == [(2, 1)] * 5 + [(1, 2)] * 5
    # the pixel walk: the area row takes a second trip, every bilinear level two or three
    B, H, W, shapes = MASKED["pixel_loop_area"][0]
    assert (H // shapes[0][0], W // shapes[0][1]) == (3, 3) and trips(B * shapes[0][0] * shapes[0][1], pixel_trip) == 2
    B, H, W, shapes = MASKED["pixel_loop_bilinear"][0]
    assert [trips(B * h * w, pixel_trip) for h, w in shapes] == [3, 2, 3]
    assert [(H / h, W / w) for h, w in shapes] == [(2.0, 2.0), (2.5, 2.5), (1.875, 1.875)]
    for h, w in shapes:                                                # no sample point on a pixel centre: m = (S > 0)
        for n_out, n_in in ((h, H), (w, W)):                           # is the same in every precision
            assert all((n_in * (2 * o + 1) - n_out) % (2 * n_out) != 0 for o in range(n_out))
            assert float(np.float32(n_in) / np.float32(n_out)) == n_in / n_out


def test_the_tile_plan_validity_holds_every_kind_of_tile():
    T = ML["kLossTile"]
    for index in range(len(MASKED["tile_plan"])):
        gt, valid, _ = masked_inputs("tile_plan", index, "v2")
        B, H, W, _ = gt.shape
        ok = ref_valid(gt.numpy(), valid.numpy())
        tiles = ok.reshape(B, H // T, T, W // T, T).transpose(0, 1, 3, 2, 4).reshape(-1, T, T)
        for k, (what, how) in enumerate(TILE_KINDS):
            n = int(tiles[k].sum())
            assert n == {"empty": 0, "full": T * T}.get(what, 1), (k, what, n)
            if what in ONE_PIXEL:
                assert tiles[k][ONE_PIXEL[what]]
        shares = tiles[len(TILE_KINDS):].reshape(len(tiles) - len(TILE_KINDS), -1).mean(axis=1)
        assert ((0.15 < shares) & (shares < 0.45)).all(), shares
        # invalid by the ground truth under a mask of ones, by NaN and by 1e10; and by the mask over ordinary values
        g = gt.numpy()
        m = valid.numpy()
        assert (np.isnan(g).any(-1) & m).any() and ((np.abs(g) > 1e9).any(-1) & m).any()
        assert (~m & np.isfinite(g).all(-1)).any()


@pytest.mark.parametrize("name,index,kind", MASKED_PARAMS)
def test_masked_rows_on_the_float64_chain(name, index, kind):
    """The oracle of the GPU module over its inputs: every level has valid and invalid pixels, the gradient is exactly 0
    at the invalid ones, and the fp32 torch chain stays within the kernels' 1e-5 of it.  Measured: at most 0.014 of the
    bound (tile_plan)."""
    gt, valid, preds = masked_inputs(name, index, kind)
    B, H, W, shapes = MASKED[name][index]
    per, counts, grads, masks_ = masked_oracle(name, index, kind)
    assert 0.2 < float(torch.from_numpy(ref_valid(gt.numpy(), valid.numpy())).float().mean()) < 0.4
    for l, (h, w) in enumerate(shapes):
        assert preds[l].shape == (B, h, w, 2) and torch.equal(preds[l], preds[l].half().float())
        assert (B * h * w * 2) % 4 == (2 if name == "bwd_scalar" else 0)
        assert 0 < int(counts[l]) == int(masks_[l].sum()) and float(per[l]) > 0
        assert int(counts[l]) < B * h * w or (H // h) * (W // w) >= 64       # a large block almost always holds a pixel
        assert not grads[l][masks_[l] == 0].any() and bool(torch.isfinite(grads[l]).all())
    obj = make_loss(kind, "channels_last")
    _, per32, counts32 = loss.multiscale_masked_torch(obj, gt, preds, valid)
    assert per32.dtype == torch.float32 and torch.equal(counts32, counts)
    err = float(((per32.double() - per).abs() / per).max())
    print("masked {} {} {}: fp32 torch chain {:.3f} of the bound".format(name, index, kind, err / 1e-5))
    assert err <= 1e-5
