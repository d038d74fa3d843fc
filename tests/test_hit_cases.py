"""The strata of tests/hit_cases.py are what they claim to be, proved on the CPU from the oracle's hits, and the float64 restatement
(tests/hit_f64.py) holds the oracle at the margin and tolerance of profiles/hits_unit/margins.txt. The device's half is
tests/test_hits_unit.py."""
import ctypes

import numpy as np
import pytest

import hit_cases as hc
import hit_f64
from conftest import scene_path

VARIANTS = ("four", "six", "far")


@pytest.fixture(scope="module")
def hits(yh, oracle):
    return {v: hc.oracle_hits(v, yh, oracle, scene_path) for v in VARIANTS + ("deep", "ties")}


def _prim_boxes(g):
    """The boxes of an object's primitives, as the upload forms them (line_bounds / triangle_bounds)."""
    p = g["positions"][g["lines"] if "lines" in g else g["triangles"]]
    r = g["radius"][g["lines"]][..., None] if "lines" in g else 0
    return np.ascontiguousarray(np.concatenate([(p - r).min(1), (p + r).max(1)], 1), np.float32)


def _leaves(yh, boxes):
    """(leaf, place in the leaf order) per box of the tree yh_bvh_build makes over (n, 6) float32 boxes."""
    lib, n = yh.load(), len(boxes)
    boxes = np.ascontiguousarray(boxes, np.float32)
    nodes, prims = np.zeros((lib.yh_bvh_build(n, yh.fptr(boxes), None, None), 8), np.float32), np.zeros(n, np.int32)
    assert lib.yh_bvh_build(n, yh.fptr(boxes), yh.fptr(nodes), yh.iptr(prims)) == len(nodes)
    start, meta = nodes[:, 6].view(np.int32), nodes[:, 7].view(np.int32)
    leaf, place = np.full(n, -1), np.full(n, -1)
    for i in np.flatnonzero((meta >> 16) & 1 == 0):
        at = np.arange(start[i], start[i] + (meta[i] & 0xffff))
        leaf[prims[at]], place[prims[at]] = i, at
    assert (leaf >= 0).all()
    return leaf, place


def _triples(s, obj, elem):
    """(number of triples, share of them whose outcome — hit or miss, object, element — changes within the triple)."""
    rows = np.flatnonzero(s.triple >= 0).reshape(-1, 3)
    assert (s.triple[rows] == s.triple[rows][:, :1]).all()
    key = np.stack([obj, elem], 1)[rows]
    return len(rows), float((key != key[:, :1]).any((1, 2)).mean())


@pytest.mark.parametrize("variant", VARIANTS)
def test_strata_are_what_they_claim(hits, yh, variant):
    obj, elem, uv, dist = hits[variant][0]
    st = hc.strata(variant)
    geo = hc.make_scenes.hits_unit_geometry(variant)
    assert len(obj) == 65536 == hc.N * len(st)  # where yh_intersect_batch takes the one-lane kernel
    for k, name in enumerate(hc.NAMES):
        sl = slice(k * hc.N, (k + 1) * hc.N)
        rate = (obj[sl] >= 0).mean()
        assert 0.05 < rate < 0.95, (name, rate)
        if name in "bcde":
            n, changed = _triples(st[name], obj[sl], elem[sl])
            assert n >= 1000 and changed >= 0.1, (name, n, changed)
    # every object is somebody's closest hit
    assert set(np.unique(obj)) == set(range(-1, len(hc.make_scenes.hits_unit_geometry(variant))))
    # ties: the twin strand (segments 16-19 and 20-23 of `strands`) and the coincident pair (triangles 37 and 130 of `tris`) are the
    # same primitive twice, so every hit on one is a hit on the other at the same t, bit for bit. Both are aimed at; the one the tree
    # tests later wins (t == tmax is accepted), every time, and its twin never does.
    for name, shape_obj, pairs in (("g", 0, [(16 + k, 20 + k) for k in range(4)]), ("b", 0, [(16 + k, 20 + k) for k in range(4)]), ("c", 2, [(37, 130)])):
        k = hc.NAMES.index(name)
        sl = slice(k * hc.N, (k + 1) * hc.N)
        won = elem[sl][obj[sl] == shape_obj]
        leaf, place = _leaves(yh, _prim_boxes(geo[shape_obj]))
        for pair in pairs:
            assert np.isin(st[name].prim, pair).any(), (name, pair)
            wins = [int((won == p).sum()) for p in pair]
            assert max(wins) >= 16 and min(wins) == 0, (name, pair, wins)
            # ... and the winner is the one tested later: the two share a leaf, and the winner stands behind its twin in the leaf order
            assert leaf[pair[0]] == leaf[pair[1]], (name, pair)
            assert place[pair[int(np.argmax(wins))]] > place[pair[int(np.argmin(wins))]], (name, pair, wins, place[list(pair)])
    # g: its 128 rows of b are hits, each of the 48 unmoved copies of them
    k = hc.NAMES.index("g")
    assert (obj[k * hc.N:(k + 1) * hc.N][np.arange(hc.N) % 64 < 48] >= 0).all()
    # the quad-only batch: every row has another tmin, and its triples decide too
    q = hc.quad_only(variant)
    assert (q.rays[:, 6] != hc.TMIN).all() and set(np.unique(q.rays[:, 6])) == {0.0, 2.0 ** -10, 1.0}
    n, changed = _triples(q, *hits[variant][1][:2])
    assert n >= 1000 and changed >= 0.1


def test_scene_numbers_are_on_the_grid():
    """Every coordinate, radius and frame entry of hits-unit is a multiple of 2^-10 below 2^6 (the rotated frame's entries and the
    translation of `far` apart), so the edge rows are exact in float32."""
    for g in hc.make_scenes.hits_unit_geometry("six"):
        vals = [g["positions"].ravel(), g["radius"]] + ([g["frame"]] if g["name"] != "d-rotated" else [g["frame"][9:]])
        for v in vals:
            v = v.astype(np.float64)
            assert np.all(v * 1024 == np.round(v * 1024)) and np.abs(v).max() < 64


def test_the_deep_chain_fills_the_stacks_past_their_windows(hits, yh):
    """Variant `deep` before any GPU run (tests/test_hits_deep.py). The upload's rule accepts the scene with 16 entries to spare:
    scene_need + 3 * depth4 + 2 <= YH_QSTACK - 16, depth4 from yh_bvh_build_wide's nodes. A numpy walk of those nodes in lane_step's
    order (hit_cases.wide_walk) over stratum x: the rays through the chain's small end stand more than 16 entries high — the LDS
    window of the one-lane kernels — when they reach their first leaf, and none stands higher than the 3 * depth4 + 2 the rule
    allows the shape. Under the chain's walk lie the ENTER entries of the objects behind it in its leaf of the scene tree, and
    hundreds of those rays end on one of them: their hit comes out of an entry that went through the overflow array."""
    from test_object_edits import _shape_levels, _stack_need, _tree
    lib = yh.load()
    lib.yhk_stack_entries.restype = ctypes.c_int
    geo = hc.make_scenes.hits_unit_geometry("deep")
    chain = geo[hc._CHAIN]
    boxes = _prim_boxes(chain)
    slots = np.zeros((lib.yh_bvh_build_wide(len(boxes), yh.fptr(boxes), 4, None), 4, 8), np.float32)
    assert lib.yh_bvh_build_wide(len(boxes), yh.fptr(boxes), 4, yh.fptr(slots)) == len(slots)
    ref, level = slots.view(np.uint32)[..., 6], np.zeros(len(slots), np.int64)
    for i in range(len(slots)):  # (breadth-first numbering: a node's children lie behind it)
        for q in ref[i][(ref[i] != 0xFFFFFFFF) & (ref[i] & 0x80000000 == 0)]:
            level[q] = level[i] + 1
    depth4 = int(level.max()) + 1
    sf = yh.SceneFile(scene_path("hits-unit", variant="deep"))
    desc = sf.desc.contents
    need = _stack_need(yh, desc, _tree(yh, desc)[1], False)
    assert depth4 == max(1 + max(0, _shape_levels(yh, desc.shapes[i]) - 2) // 2 for i in range(desc.num_shapes))  # the chain is the deepest shape
    sf.close()
    print("deep: depth4", depth4, "stack_need", need, "of", lib.yhk_stack_entries())
    assert need + 16 <= lib.yhk_stack_entries() == 96
    rays = hc.deep_rays()[:hc.N].astype(np.float64)
    f = chain["frame"].astype(np.float64).reshape(4, 3)
    top, first = hc.wide_walk(slots, (rays[:, 0:3] - f[3]) @ np.linalg.inv(f[:3]), rays[:, 3:6] @ np.linalg.inv(f[:3]))
    print("deep: the highest stack", int(top.max()), "rays above 16 at their first leaf", int((first > 16).sum()))
    assert (first > 16).sum() >= hc.N // 2 and top.max() <= 3 * depth4 + 2
    # the objects entered after the chain from its leaf of the scene tree, and the rays that end on them from above the window
    leaf, place = _leaves(yh, np.array([np.concatenate(b) for b in hc.world_boxes(geo)]))
    behind = [k for k in range(len(geo)) if leaf[k] == leaf[hc._CHAIN] and place[k] > place[hc._CHAIN]]
    assert behind, (leaf, place)
    obj = hits["deep"][0][0][:hc.N]
    assert (np.isin(obj, behind) & (first > 16)).sum() >= 500, (behind, np.unique(obj[first > 16], return_counts=True))


def _wide(yh, boxes, width):
    """yh_bvh_build_wide's nodes over (n, 6) float32 boxes: (nodes, width, 8) float32."""
    lib, boxes = yh.load(), np.ascontiguousarray(boxes, np.float32)
    slots = np.zeros((lib.yh_bvh_build_wide(len(boxes), yh.fptr(boxes), width, None), width, 8), np.float32)
    assert lib.yh_bvh_build_wide(len(boxes), yh.fptr(boxes), width, yh.fptr(slots)) == len(slots)
    return slots


def _wide_depth(slots):
    """The levels of wide nodes, from the nodes themselves (breadth-first numbering: a node's children lie behind it)."""
    ref, level = slots.view(np.uint32)[..., 6], np.zeros(len(slots), np.int64)
    for i in range(len(slots)):
        for q in ref[i][(ref[i] != 0xFFFFFFFF) & (ref[i] & 0x80000000 == 0)]:
            level[q] = level[i] + 1
    return int(level.max()) + 1


def _wide_node_of_leaf(slots):
    """first place of a leaf in the leaf order -> the wide node that holds it in a slot."""
    ref = slots.view(np.uint32)[..., 6]
    node, _ = np.nonzero((ref & 0x80000000 != 0) & (ref != 0xFFFFFFFF))
    return {int(r & 0x07FFFFFF): int(k) for k, r in zip(node, ref[(ref & 0x80000000 != 0) & (ref != 0xFFFFFFFF)])}


def _object_space(g, rays):
    f = g["frame"].astype(np.float64).reshape(4, 3)
    return (rays[:, 0:3].astype(np.float64) - f[3]) @ np.linalg.inv(f[:3]), rays[:, 3:6].astype(np.float64) @ np.linalg.inv(f[:3])


def test_ties_are_shared_across_leaves_and_the_visiting_order_decides(hits, yh):
    """Variant `ties` before any GPU run. A primitive's twins (make_scenes._hits_ties: the very same record) are tested with the very same
    arithmetic: a hit on one is a hit on each at the same t as bits, whatever tmax has shrunk to among them (t == tmax is accepted). So a
    row's closest hit is shared across leaves wherever the winner's twins lie in two or more binary leaves (yh_bvh_build), and across slots
    of ONE wide node wherever two of those leaves are slots of one 8- or 16-wide node (yh_bvh_build_wide). Who wins is the visiting
    order's to say: on the rows aimed at the stack at least three copies win, and another one when the ray runs against x."""
    obj, elem, uv, dist = hits["ties"][0]
    s, geo = hc.ties(), hc.make_scenes.hits_unit_geometry("ties")
    cross, same = np.zeros(hc.N, bool), {8: np.zeros(hc.N, bool), 16: np.zeros(hc.N, bool)}
    for name, k in hc.TIES_OBJECTS.items():
        g = geo[k]
        leaf, place = _leaves(yh, _prim_boxes(g))
        start = {l: int(place[leaf == l].min()) for l in np.unique(leaf)}
        node_of = {w: _wide_node_of_leaf(_wide(yh, _prim_boxes(g), w)) for w in (8, 16)}
        print(f"ties {name}: {len(leaf)} primitives in {len(start)} leaves, {len(set(node_of[8].values()))} 8-wide and {len(set(node_of[16].values()))} 16-wide nodes with leaves")
        for e in np.unique(elem[obj == k]):
            leaves = np.unique(leaf[g["twin"] == g["twin"][e]])
            rows = (obj == k) & (elem == e)
            cross |= rows & (len(leaves) >= 2)
            for w in (8, 16):
                nodes = [node_of[w][start[l]] for l in leaves]
                same[w] |= rows & (len(nodes) > len(set(nodes)))
    print("ties: rows whose closest hit is shared across leaves", int(cross.sum()), "across slots of one 8-wide node", int(same[8].sum()), "of one 16-wide node", int(same[16].sum()))
    assert cross.sum() >= 1000 and same[8].sum() >= 256 and same[16].sum() >= 256
    for name in ("stack", "plates"):
        k = hc.TIES_OBJECTS[name]
        rows = (s.object == k) & (obj == k)
        dx = s.rays[:, 3]
        won = {sign: np.unique(elem[rows & (dx * sign > 0)], return_counts=True) for sign in (1, -1)}
        print(f"ties {name}: winners with the ray along +x", dict(zip(*won[1])), "against x", dict(zip(*won[-1])))
        assert len(np.unique(elem[rows])) >= 3
        assert won[1][0][won[1][1].argmax()] != won[-1][0][won[-1][1].argmax()]  # the copy that wins most often changes with the sign
        assert min(won[1][1].max(), won[-1][1].max()) >= 64


def test_the_walk_at_widths_8_and_16(hits, yh):
    """hit_cases.wide_walk_any — the walk at widths 4, 8 and 16 with the rank rules of csrc/dev_trace.h — is the 4-wide walk on `deep`, finds
    the leaf runs a leaf group looks for on top of the stack (`ties`, stratum g of `four`), and on stratum x of `deep` never stands
    higher than the shape's part of stack_needs: 7 * depth8 + 2 and 15 * depth16 + 2, the depths from the wide nodes themselves. A
    column that overruns its entries writes into its neighbour's."""
    geo = hc.make_scenes.hits_unit_geometry("deep")
    chain = geo[hc._CHAIN]
    o, d = _object_space(chain, hc.deep_rays()[:hc.N])
    top4, first4 = hc.wide_walk(_wide(yh, _prim_boxes(chain), 4), o, d)
    heights = {}
    for width, per_level in ((4, 3), (8, 7), (16, 15)):
        slots = _wide(yh, _prim_boxes(chain), width)
        top, first, run, under = hc.wide_walk_any(slots, o, d)
        if width == 4:
            assert np.array_equal(top, top4) and np.array_equal(first, first4)
        depth = _wide_depth(slots)
        heights[width] = (int(top.max()), depth, per_level * depth + 2)
        assert top.max() <= per_level * depth + 2, heights
    print("deep: the highest stack, the depth in wide nodes and the bound per width", heights)
    assert heights[8][0] > 16 and heights[16][0] > 16  # (the wide stacks stand high too)
    # leaf runs on top of the stack at a ray's first leaf
    tg, fg = hc.make_scenes.hits_unit_geometry("ties"), hc.make_scenes.hits_unit_geometry("four")
    batches = [(tg[k], hc.ties().rays[hc.ties().object == k]) for k in hc.TIES_OBJECTS.values()]
    g = hc.strata("four")["g"]
    batches.append((fg[0], g.rays[g.object == 0]))
    for width in (8, 16):
        runs, unders = [], []
        for gk, rays in batches:
            top, first, run, under = hc.wide_walk_any(_wide(yh, _prim_boxes(gk), width), *_object_space(gk, rays))
            runs.append(run[first >= 0]), unders.append(under[first >= 0])
        run, under = np.concatenate(runs), np.concatenate(unders)
        count = {"0": int((run == 0).sum()), "1": int((run == 1).sum()), "2": int((run == 2).sum()), "3+": int((run >= 3).sum()),
                 "ended by a node": int(((run >= 1) & under).sum()), "ended by the bottom": int(((run >= 1) & ~under).sum())}
        print(f"width {width}: rays by leaf entries on top of the stack at their first leaf", count)
        assert min(count.values()) >= 64, (width, count)


@pytest.mark.parametrize("variant", VARIANTS + ("deep", "ties"))
def test_float64_holds_the_oracle(hits, variant):
    """No tree, box or cull of the oracle loses a hit that float64 finds with a margin (hit_f64.compare), and the constants are the
    measured ones: M is the smallest power of two that holds, T twice the largest error on stratum a. The cap that keeps the bar honest:
    at most 1 % of stratum a is at or below M on `four` and `six`."""
    share = hit_f64.compare(variant, hits[variant][0])
    m, t, _ = hit_f64.measure(variant, hits[variant][0])
    assert m == hit_f64.M[variant], (m, hit_f64.M[variant])
    assert t <= hit_f64.T[variant] <= 1.01 * t, (t, hit_f64.T[variant])
    print(variant, "rows at or below M:", {k: f"{100 * v:.2f}%" for k, v in share.items()})
    if variant in ("four", "six"):
        assert share["a"] <= 0.01, share
