"""GPU: opq_remove (IVFOPQ::LoadIndex + RemoveVideos + SaveIndex) on the reference's own five feature files: the index with
videos 1 and 3 taken out is, byte for byte and by name, the index opq_index builds over the three kept files alone, and opq_query
prints the same scores on both."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
NAMES = ["6231519245", "6231075428", "6230951284", "6230880830", "6231307582"]  # opq/data/5_feats_list.txt order


def run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_opq_remove_cli_equals_an_index_of_the_kept_files(tmp_path, golden):
    from oracle import binding as ob
    for exe in ("opq_index", "opq_remove", "opq_query"):
        assert os.path.exists(os.path.join(BIN, exe)), "host CLIs not built: __graft_entry__.build()"
    g = golden.opq["opq_real_q9"]
    model = str(tmp_path / "model.bin")
    ob.write_opq_model(model, g["coarse"], g["books"], g["perm"])
    feat = [os.path.join(golden.dir, "opq_data", "db", n + "_feat.bin") for n in NAMES]
    gone = [1, 3]
    (tmp_path / "all.txt").write_text("\n".join(feat) + "\n")
    (tmp_path / "kept.txt").write_text("\n".join(f for v, f in enumerate(feat) if v not in gone) + "\n")
    for d in ("all", "kept", "removed"):
        (tmp_path / d).mkdir()
    run([os.path.join(BIN, "opq_index"), model, str(tmp_path / "all.txt"), str(tmp_path / "all")], cwd=str(tmp_path))
    run([os.path.join(BIN, "opq_index"), model, str(tmp_path / "kept.txt"), str(tmp_path / "kept")], cwd=str(tmp_path))
    (all_name,) = os.listdir(tmp_path / "all")
    out = run([os.path.join(BIN, "opq_remove"), model, str(tmp_path / "all" / all_name), str(tmp_path / "removed")] + [str(v) for v in gone],
              cwd=str(tmp_path))
    assert "of 2 videos, 3 videos left" in out, out
    (kept_name,) = os.listdir(tmp_path / "kept")
    assert os.listdir(tmp_path / "removed") == [kept_name] and kept_name != all_name and "_db_3_" in kept_name
    want = (tmp_path / "kept" / kept_name).read_bytes()
    got = (tmp_path / "removed" / kept_name).read_bytes()
    assert len(got) == len(want) and got == want, "index after opq_remove differs from opq_index over the kept files"
    assert len(want) < len((tmp_path / "all" / all_name).read_bytes())
    # the same scores from both
    q = os.path.join(golden.dir, "opq_data", "query", "6231519245_feat.bin")
    res = []
    for d in ("kept", "removed"):
        run([os.path.join(BIN, "opq_query"), model, str(tmp_path / d / kept_name), str(tmp_path / ("res_%s.txt" % d)), q, "--nearest", "3",
             "--show", "3"], cwd=str(tmp_path))
        res.append((tmp_path / ("res_%s.txt" % d)).read_text())
    assert res[0] == res[1] and res[0].splitlines()[1].split()[0] == NAMES[0] + "_feat"
