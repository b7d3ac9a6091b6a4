"""The fused SVCE decoder without a GPU: the argument and geometry checks of svc_hip_decode_entropy_frames that answer before any
device work, their order, and its workspace query."""

from scalable_video_codec_amd import native


def _decode(lib, w, h, bw, bh, mbw, mbh, fg=1, bg=640, dw=0, dh=0, n=2, ws=1 << 30):
    return lib.svc_hip_decode_entropy_frames(None, 0, None, n, w, h, bw, bh, mbw, mbh, fg, bg, None, None, ws, None, None, dw, dh,
                                             None, None)


def _err(lib):
    return lib.svc_hip_last_error().decode()


def test_refusals_answer_without_a_device():
    lib = native.load()
    # transform blocks the reconstruction does not take (the format does)
    assert _decode(lib, 96, 96, 12, 12, 48, 48) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in _err(lib)
    assert _decode(lib, 64, 64, 4, 4, 16, 16) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in _err(lib)
    assert _decode(lib, 64, 64, 8, 16, 16, 16) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in _err(lib)
    # a width that is not whole 16-pixel segments
    assert _decode(lib, 72, 64, 8, 8, 8, 8) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in _err(lib)
    # a step of 0
    assert _decode(lib, 64, 64, 8, 8, 16, 16, fg=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in _err(lib)
    assert _decode(lib, 64, 64, 8, 8, 16, 16, bg=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in _err(lib)
    # a display larger than the frame, or with one side only
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=65, dh=64) == native.SVC_ERR_INVALID_ARG and "display" in _err(lib)
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=64, dh=65) == native.SVC_ERR_INVALID_ARG and "display" in _err(lib)
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=0, dh=32) == native.SVC_ERR_INVALID_ARG and "display" in _err(lib)
    # more frames than a call takes
    assert _decode(lib, 64, 64, 8, 8, 16, 16, n=65536) == native.SVC_ERR_UNSUPPORTED and "65535" in _err(lib)
    # a short workspace, then the pointers
    need = native.decode_entropy_workspace_bytes(2, 64, 64, 8, 16)
    assert _decode(lib, 64, 64, 8, 8, 16, 16, ws=need - 1) == native.SVC_ERR_INVALID_ARG and "workspace" in _err(lib)
    assert _decode(lib, 64, 64, 8, 8, 16, 16, ws=need) == native.SVC_ERR_INVALID_ARG and "null pointer" in _err(lib)
    assert _decode(lib, 64, 64, 16, 16, 32, 32, dw=64, dh=64) == native.SVC_ERR_INVALID_ARG and "null pointer" in _err(lib)


def test_checks_come_in_the_order_of_the_other_stream_entry_points():
    """Each call is wrong in two ways; the earlier check answers: the format's geometry, the reconstruction's geometry, steps,
    display size, limits, workspace, pointers."""
    lib = native.load()
    # the format's own geometry before the reconstruction's
    assert _decode(lib, 100, 64, 12, 12, 16, 16) == native.SVC_ERR_INVALID_ARG and "not divisible" in _err(lib)
    assert _decode(lib, 64, 64, 8, 8, 12, 16, fg=0) == native.SVC_ERR_INVALID_ARG and "multiple of the tile" in _err(lib)
    # geometry before steps
    assert _decode(lib, 96, 96, 12, 12, 48, 48, fg=0) == native.SVC_ERR_UNSUPPORTED
    assert _decode(lib, 72, 64, 8, 8, 8, 8, bg=0) == native.SVC_ERR_UNSUPPORTED
    # steps before the display size
    assert _decode(lib, 64, 64, 8, 8, 16, 16, fg=0, dw=65, dh=64) == native.SVC_ERR_INVALID_ARG and "steps" in _err(lib)
    # the display size before the limits
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=65, dh=64, n=65536) == native.SVC_ERR_INVALID_ARG and "display" in _err(lib)
    # the limits before the workspace
    assert _decode(lib, 64, 64, 8, 8, 16, 16, n=65536, ws=0) == native.SVC_ERR_UNSUPPORTED and "65535" in _err(lib)
    # the workspace before the pointers
    assert _decode(lib, 64, 64, 8, 8, 16, 16, ws=0) == native.SVC_ERR_INVALID_ARG and "workspace" in _err(lib)
    # the same order for an empty batch, which is then accepted before the pointers
    assert _decode(lib, 96, 96, 12, 12, 48, 48, n=0) == native.SVC_ERR_UNSUPPORTED
    assert _decode(lib, 72, 64, 8, 8, 8, 8, n=0) == native.SVC_ERR_UNSUPPORTED
    assert _decode(lib, 64, 64, 8, 8, 16, 16, fg=0, n=0) == native.SVC_ERR_INVALID_ARG
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=65, dh=1, n=0) == native.SVC_ERR_INVALID_ARG


def test_an_empty_batch_with_null_pointers_is_ok():
    lib = native.load()
    assert _decode(lib, 64, 64, 8, 8, 16, 16, n=0, ws=0) == native.SVC_OK
    assert _decode(lib, 224, 64, 16, 16, 32, 32, dw=48, dh=40, n=0, ws=0) == native.SVC_OK


def test_workspace_bytes():
    # refused geometries: 0
    assert native.decode_entropy_workspace_bytes(2, 96, 96, 12, 48) == 0
    assert native.decode_entropy_workspace_bytes(2, 64, 64, 4, 16) == 0
    assert native.decode_entropy_workspace_bytes(2, 64, 64, (8, 16), 16) == 0
    assert native.decode_entropy_workspace_bytes(2, 72, 64, 8, 8) == 0
    assert native.decode_entropy_workspace_bytes(2, 100, 64, 8, 16) == 0
    assert native.decode_entropy_workspace_bytes(2, 64, 64, 8, 12) == 0
    assert native.decode_entropy_workspace_bytes(65536, 64, 64, 8, 16) == 0
    assert native.decode_entropy_workspace_bytes(0, 64, 64, 8, 16) == 0  # an empty batch needs none
    # accepted ones: positive, monotone in n_frames, and within the entropy coder's own workspace (it holds the same index scan)
    for w, h, b, mvb in [(1920, 1088, 8, 16), (320, 48, 8, 16), (224, 64, 16, 32), (208, 64, 16, 16)]:
        sizes = [native.decode_entropy_workspace_bytes(n, w, h, b, mvb) for n in (1, 2, 3, 16, 17, 64)]
        assert sizes[0] > 0 and all(a <= c for a, c in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert sizes[3] <= native.entropy_workspace_bytes(16, w, h, b, mvb)
