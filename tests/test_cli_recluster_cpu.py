"""CPU only: the options of `phage_filter recluster` are checked before any device is used (status 101, a message that names the
option, nothing written), and the usage text lists the command, its options, MERGES.tsv's columns and `build --cluster`."""
import os
import subprocess

import cluster_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "phagefilter_amd", "phage_filter")
# (no device may be touched: one that is asked for does not exist)
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def refused(tmp_path, *args):
    before = sorted(os.listdir(tmp_path))
    p = subprocess.run([CLI, "recluster", *args], capture_output=True, text=True, env=ENV, timeout=60, cwd=str(tmp_path))
    assert p.returncode == 101, (args, p.returncode, p.stderr)
    assert sorted(os.listdir(tmp_path)) == before, "refused before anything is written"
    return p.stderr


def test_db_path_and_out_are_required(tmp_path):
    db, out = str(tmp_path / "no_such_db"), str(tmp_path / "new")
    assert "--db-path" in refused(tmp_path, "-o", out)
    assert "--out" in refused(tmp_path, "-d", db)
    err = refused(tmp_path, "-d", db, "-o", out, "--device", "x")
    assert "'--device'" in err and "'x'" in err, err
    assert "--reads" in refused(tmp_path, "-d", db, "-o", out, "--reads", "x")
    assert "--merges" in refused(tmp_path, "-d", db, "-o", out, "--merges")
    assert "'--merges'" in refused(tmp_path, "-d", db, "-o", out, "--merges", "")
    assert "'--out'" in refused(tmp_path, "-d", db, "--out=")


def test_out_must_not_be_the_database(tmp_path):
    db = tmp_path / "db"
    db.mkdir()
    (tmp_path / "link").symlink_to(db)
    for d, o in ((str(db), str(db)), (str(db), str(db) + "/"), ("db", "./db"), (str(db), str(tmp_path / "link")), ("db", str(tmp_path / "link" / ".." / "db")),
                 (str(tmp_path / "gone"), str(tmp_path / "gone") + "//")):
        err = refused(tmp_path, "-d", d, "-o", o, "--merges", str(tmp_path / "m.tsv"))
        assert "'--out'" in err and "--db-path" in err, (d, o, err)
    assert os.listdir(db) == []


def test_build_takes_cluster_and_checks_its_options_first(tmp_path):
    p = subprocess.run([CLI, "build", "--cluster", "-d", str(tmp_path / "db")], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101 and "--genomes" in p.stderr and not os.path.exists(tmp_path / "db"), p.stderr
    p = subprocess.run([CLI, "build", "--cluster=1", "-g", "x", "-d", str(tmp_path / "db"), "-k", "z"], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 101 and "kmer-size" in p.stderr and not os.path.exists(tmp_path / "db"), p.stderr


def test_usage_lists_the_command():
    p = subprocess.run([CLI], capture_output=True, text=True, env=ENV, timeout=60)
    text = p.stderr + p.stdout
    assert "\n  recluster " in text
    assert "recluster -d <DB> -o <NEWDB> [--merges <FILE>] [--device <N>]" in text and "build --cluster" in text
    assert cluster_ref.HEADER.replace("\t", "<TAB>") in text
