"""The build's "is this object stale" test reads the compiler's dependency lists (soccerdiffusion_amd/build.py, _deps): the lists name the
project's files relative to csrc/, so they hold wherever the tree lies, and a list that another tree (or another unit) wrote counts as
missing.  Nothing is compiled here."""

import os

from soccerdiffusion_amd import build


def _write_list(monkeypatch, tmp_path, text):
    monkeypatch.setattr(build, "LIB_DIR", str(tmp_path))
    src = os.path.join(build.CSRC, "sd_head.hip")
    with open(build._dep_file(src), "w") as f:
        f.write(text)
    return src


def test_relative_list_resolves_inside_this_tree(monkeypatch, tmp_path):
    src = _write_list(monkeypatch, tmp_path, "sd_head.o.tmp: sd_head.hip \\\n  /opt/rocm/include/hip/hip_runtime.h sd_common.h \\\n"
                                             "  ../../include/soccerdiffusion_hip.h\n")
    assert build._deps(src) == [src, os.path.join(build.CSRC, "sd_common.h"), os.path.join(build.REPO, "include", "soccerdiffusion_hip.h"),
                                os.path.abspath(build.__file__)]
    assert all(os.path.exists(p) for p in build._deps(src))


def test_list_written_in_another_tree_counts_as_missing(monkeypatch, tmp_path):
    src = _write_list(monkeypatch, tmp_path, "sd_head.o.tmp: /somewhere/else/soccerdiffusion_amd/csrc/sd_head.hip \\\n"
                                             "  /somewhere/else/soccerdiffusion_amd/csrc/sd_common.h /opt/rocm/include/hip/hip_runtime.h\n")
    assert build._deps(src) is None
    assert build._obj_stale(src)
    assert build.is_stale()


def test_list_of_another_unit_or_no_list_counts_as_missing(monkeypatch, tmp_path):
    src = _write_list(monkeypatch, tmp_path, "sd_swin.o.tmp: sd_swin.hip sd_common.h\n")
    assert build._deps(src) is None
    os.remove(build._dep_file(src))
    assert build._deps(src) is None


def test_compile_command_names_project_files_relative_to_csrc():
    cmd = build.compile_cmd(os.path.join(build.CSRC, "sd_traj.hip"), "/tmp/x.o")
    assert cmd[cmd.index("-c") + 1] == "sd_traj.hip" and cmd[cmd.index("-I") + 1] == os.path.join("..", "..", "include")
    assert cmd[cmd.index("-MF") + 1] == "/tmp/x.o.d"
    assert "-packed-fp32-ops" in cmd   # the step kernels' unit keeps its flag (EXTRA_FLAGS)
