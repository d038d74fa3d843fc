"""What yh_upload_scene lays out is what it laid out before its stages were split: tests/golden/upload_layout.json (tools/upload_layout.py,
written by the commit its header names) holds, for five small scenes, where every shape's wide nodes sit in the traversal array, the
light list, and the forms the scene table settles on. The arrays' contents are held bit for bit elsewhere (the hit suites, the light and
edit suites); this is the layout they sit in."""
import json

import pytest

import upload_layout
from conftest import scene_path


def test_golden_file_names_its_commit_and_every_scene():
    doc = json.load(open(upload_layout.GOLDEN))
    assert "commit 308c4a2" in doc["header"]
    assert sorted(doc["scenes"]) == sorted(tag for tag, *_ in upload_layout.SCENES)
    fur = doc["scenes"]["fur-field"]["yh_shape_nodes"]
    assert min(s["offset"][0] for s in fur) > 4 * 339  # (its scene level is walked as wide nodes: their room is in front of everything)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,name,kw,with_maps", upload_layout.SCENES, ids=[s[0] for s in upload_layout.SCENES])
def test_upload_lays_out_what_the_golden_file_holds(ctx, yh, tag, name, kw, with_maps):
    want = json.load(open(upload_layout.GOLDEN))["scenes"][tag]
    got = upload_layout.layout(ctx, yh, scene_path(name, **kw), with_maps)
    assert got == want
