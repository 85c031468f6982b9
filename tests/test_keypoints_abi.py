"""CPU: the keypoint NMS / row gather entry points (include/dh3d_hip.h, csrc/keypoints.hip) are exported and reject bad
arguments with status codes before touching the GPU; the workspace size is a host-only function of the shape."""
import ctypes

NEW_SYMBOLS = ("dh3d_keypoint_nms", "dh3d_keypoint_nms_workspace_bytes", "dh3d_gather_rows")


def test_keypoint_symbols_exported():
    from dh3d_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name


def _nms(lib, score, nn, dist, count, inds, ws, K=50, M=512, ws_bytes=1 << 30, B=2, N=1000):
    return lib.dh3d_keypoint_nms(score, 132, 1, nn, dist, None, B, N, K, 0.5, 0.01, M, 1, count, inds, ws, ws_bytes, None)


def test_keypoint_nms_bad_arguments_are_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, p = None, 256  # (a non-null fake pointer: every check below fails before a launch)
    assert _nms(lib, z, p, p, p, p, p) == 1          # null score
    assert _nms(lib, p, z, p, p, p, p) == 1          # null nn
    assert _nms(lib, p, p, z, p, p, p) == 1          # null dist
    assert _nms(lib, p, p, p, z, p, p) == 1          # null count
    assert _nms(lib, p, p, p, p, z, p) == 1          # null inds
    assert _nms(lib, p, p, p, p, p, z) == 1          # null workspace
    assert _nms(lib, p, p, p, p, p, p, M=0) == 1     # M = 0
    assert _nms(lib, p, p, p, p, p, p, K=0) == 1     # K = 0
    assert _nms(lib, p, p, p, p, p, p, B=0) == 1     # B = 0
    assert _nms(lib, p, p, p, p, p, p, N=0) == 1     # N = 0
    assert _nms(lib, p, p, p, p, p, p, M=4097) == 2  # beyond the winners' LDS sort
    assert _nms(lib, p, p, p, p, p, p, K=65) == 2    # beyond the kNN kernels' limit
    assert _nms(lib, p, p, p, p, p, p, ws_bytes=16) == 1  # workspace too small
    assert lib.dh3d_keypoint_nms(p, 0, 1, p, p, None, 2, 1000, 50, 0.5, 0.01, 512, 1, p, p, p, 1 << 30, None) == 1  # stride 0


def test_gather_rows_bad_arguments_are_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, p = None, 256
    assert lib.dh3d_gather_rows(z, 2, 100, 132, p, p, 8, p, None) == 1
    assert lib.dh3d_gather_rows(p, 2, 100, 132, z, p, 8, p, None) == 1
    assert lib.dh3d_gather_rows(p, 2, 100, 132, p, z, 8, p, None) == 1
    assert lib.dh3d_gather_rows(p, 2, 100, 132, p, p, 8, z, None) == 1
    assert lib.dh3d_gather_rows(p, 2, 100, 0, p, p, 8, p, None) == 1
    assert lib.dh3d_gather_rows(p, 2, 100, 132, p, p, 0, p, None) == 1


def test_keypoint_workspace_bytes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    ws = lib.dh3d_keypoint_nms_workspace_bytes
    sizes = [ws(4, n, 512) for n in (1, 49, 256, 257, 4096, 16384, 100000)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)  # grows with N
    assert ws(4, 16384, 512) >= 4 * 16384 * 12  # a' + a 64-bit key per point
    assert ws(8, 16384, 512) > ws(4, 16384, 512)
    assert ws(4, 16384, 0) == 0 and ws(4, 16384, 4097) == 0 and ws(0, 16384, 512) == 0  # shapes not served
