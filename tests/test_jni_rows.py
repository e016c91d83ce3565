"""exportRows of the JNI glue (jni/deltareplay_jni.c) on the mock JNIEnv, as its own sanitized
program (tests/native/jni_mock_rows.c): the selection's 24 buffers and the range handle come back; a
null `rows` raises IllegalArgumentException before the library is called; a handleOut without a
slot is refused; a column over 2^31 - 1 bytes is refused and the range released; a buffer the JVM
refuses releases the range too; no scenario makes a JNI call while an exception is pending."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLUE = os.path.join(ROOT, "jni", "deltareplay_jni.c")
MOCK = os.path.join(ROOT, "tests", "native", "jni_mock_rows.c")
SCENARIOS = ["export_rows_columns", "export_rows_null_rows", "export_rows_needs_handle",
             "export_rows_over_2gib_refused", "export_rows_buffer_failure_releases", "export_rows_empty_selection"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_export_rows_on_a_mock_jni_env(tmp_path):
    mock_src = open(MOCK).read()
    defined = set(re.findall(r"^\S[^(\n]*\b(dr_\w+)\(", mock_src, re.M))
    assert {"dr_state_export_rows", "dr_range_release"} <= defined
    called = set(re.findall(r"\b(dr_\w+)\(", open(GLUE).read()))
    assert "dr_state_export_rows" in called
    gen = tmp_path / "gen_stubs.c"
    gen.write_text("".join("int %s() { return 15; }\n" % f for f in sorted(called - defined)))
    exe = tmp_path / "jni_mock_rows"
    inc = ["-I", os.path.join(ROOT, "tests", "native", "jni_min"), "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "native")]
    r = subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wno-builtin-declaration-mismatch"] + inc + [GLUE, MOCK, str(gen), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines == [s + " ok" for s in SCENARIOS], run.stdout + run.stderr


def test_export_rows_is_bound_in_scala():
    scala = open(os.path.join(ROOT, "jni", "DeltaReplayNative.scala")).read()
    assert re.search(r"@native def exportRows\(state: Long, which: Int, rows: Array\[Long\], handleOut: Array\[Long\]\): "
                     r"Array\[ByteBuffer\]", scala)
