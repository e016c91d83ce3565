"""Folded punctuation in the K1 line walker on the GPU: the corpus of tests/test_json_fold.py written
as commit files, parsed record for record against the PERMISSIVE-reader restatement
(tests/test_json_lane.py `expected`: Python's json plus the oracle's unwrap rules) through

 * the bulk kernel (k_json_lines<false>, the per-lane walker with the LDS token buffer, and
   k_json_hard for the lines it defers): one commit of many index blocks, the window and token-buffer
   cases repeated behind a line of 0..15 bytes so that every line meets every 16-byte window phase;
 * the small-segment path (k_json_lines<true>: stage, token tape, tape walk): commits of at most 64
   lines in one 16 KiB index block, one of them without its final newline.

Both run on the default library and, in a child process, on the library built with the LDS index
checks (DR_LIB, as tests/test_gpu_bounds.py selects it), which must report no index out of range."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def corpus():
    from tests.test_json_fold import fold_corpus
    lines = [l for l in fold_corpus() if b"\n" not in l]
    assert len(lines) > 4000
    return lines


_EXPECTED = {}


def _expected(line):
    from tests.test_json_lane import expected
    if line not in _EXPECTED:
        _EXPECTED[line] = expected(line)
    return _EXPECTED[line]


def _parse(engine, body):
    staged = engine.stage_files([(0, 0, 0, body)])
    try:
        return staged.parse_lines()
    finally:
        staged.release()


def _compare(lines, got):
    from tests.test_gpu_edge_cases import _device_view
    assert len(got) == len(lines)
    for line, rec in zip(lines, got):
        assert rec["line"] == line
        assert _device_view(rec) == _expected(line), line


def test_bulk_kernel(engine, corpus):
    from tests.test_json_fold import buffer_cases, window_cases
    lines = list(corpus)
    phased = window_cases() + buffer_cases()
    for skew in range(16):
        lines.append(b"x" * skew)  # an error line that shifts everything after it
        lines.extend(phased)
    body = b"".join(l + b"\n" for l in lines)
    assert len(lines) > 256 and len(body) >= 2 * 16384  # the bulk walker's segment, several index blocks
    _compare(lines, _parse(engine, body))


def test_small_segments(engine, corpus):
    chunks, cur, size = [], [], 0
    for line in corpus:
        if len(line) + 1 > 16384:
            continue
        if len(cur) == 64 or size + len(line) + 1 > 16384:
            chunks.append(cur)
            cur, size = [], 0
        cur.append(line)
        size += len(line) + 1
    chunks.append(cur)
    assert sum(len(c) for c in chunks) == len(corpus)
    for k, lines in enumerate(chunks):
        body = b"".join(l + b"\n" for l in lines)
        if k % 7 == 3 and lines[-1]:
            body = body[:-1]  # a commit whose last line has no newline
        _compare(lines, _parse(engine, body))


def test_lines_over_the_token_offset_limit(engine):
    """Lines over 65535 bytes (k_json_hard's General walker): members, null tag values and keys behind offset
    65535 and behind 2 * 65536, between ordinary lines, in one commit and each in a commit of its own."""
    from tests.test_json_fold import ADD, REMOVE, over_the_line_limit_cases
    cases = over_the_line_limit_cases()
    lines = [ADD]
    for line in cases:
        lines += [line, REMOVE, ADD]
    _compare(lines, _parse(engine, b"".join(l + b"\n" for l in lines)))
    for line in cases[:9]:
        _compare([line], _parse(engine, line + b"\n"))


def test_both_paths_on_the_bounds_build():
    lib = os.path.join(ROOT, "delta_amd", "libdeltareplay_bounds.so")
    assert os.path.exists(lib), "make builds libdeltareplay_bounds.so"
    if os.environ.get("DR_LIB") == "libdeltareplay_bounds.so":
        return  # this is the child
    sel = ["tests/test_gpu_json_fold.py::test_bulk_kernel", "tests/test_gpu_json_fold.py::test_small_segments"]
    env = dict(os.environ, DR_LIB="libdeltareplay_bounds.so")
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"] + sel,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "2 passed" in out
    hits = [l for l in out.splitlines() if "LDS-BOUNDS" in l]
    assert not hits, hits[:20]
