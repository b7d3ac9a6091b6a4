"""In-tree build of the native libraries (hipcc cross-compiles gfx950 without a GPU).

  libsvc_hip.so     HIP kernels + the C ABI of include/svc_hip.h
  libsvc_motion.so  C++ wrappers with the reference's own signatures
                    (include/svc/motion.hpp), on top of the C ABI
  libsvc_opencv_compat.so  compat/opencv2: the OpenCV-shaped adapter the reference's own
                    encoder application compiles against, on top of the C ABI

Both land next to this file; they are git-ignored but travel to the GPU box.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import shutil
import subprocess
import sys
from typing import List

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJ = os.path.join(PKG, "_obj")
LIB_HIP = os.path.join(PKG, "libsvc_hip.so")
LIB_MOTION = os.path.join(PKG, "libsvc_motion.so")

HIP_SOURCES = ["capi.hip", "hbma_wave.hip", "hbma_fused.hip", "hbma_fused8.hip", "hbma_fused32.hip", "hbma_tiled.hip", "dct.hip", "dct_pack.hip", "ransac.hip", "luma_pyramid.hip", "segment.hip", "wire.hip", "idct.hip", "probe.hip", "comm.hip", "global_motion.hip", "imageops.hip", "levels.hip", "records.hip", "entropy.hip"]
HOST_SOURCES = [os.path.join("host", "motion_hip.cpp")]

# -ffp-contract=off: the reference's float expressions (RANSAC inlier test, quant) are
# evaluated without FMA on baseline x86-64; the DCT asks for its FMAs explicitly.
# -Wno-inline-asm: hbma_tiled.hip's LDS-DMA asm names m0 in its clobber list ON PURPOSE (it writes m0; the backend must not
# merge one of its own m0 initialisations across it); LLVM answers every such asm with "clobber list contains reserved registers".
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
               "-Wall", "-Wno-unused-function", "-Wno-inline-asm", f"-I{INCLUDE}", f"-I{CSRC}"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the MI355X path cannot be built")
    return exe


def _newer(target: str, deps: List[str]) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _headers() -> List[str]:
    """Every header a native source may include: listed by directory, so a new one cannot be left out and keep a stale library."""
    pats = [(CSRC, "*.hpp"), (CSRC, "*.inc"), (os.path.join(CSRC, "host"), "*.hpp"), (INCLUDE, "*.h"), (os.path.join(INCLUDE, "svc"), "*.hpp")]
    return sorted(f for d, pat in pats for f in glob.glob(os.path.join(d, pat)))


def _run(cmd: List[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise RuntimeError(f"build step failed: {os.path.basename(cmd[-1])}")


def build_hip(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJ, exist_ok=True)
    headers = _headers()
    jobs, objs = [], []
    for s in HIP_SOURCES:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or not _newer(obj, [src] + headers):
            jobs.append([_hipcc(), *HIPCC_FLAGS, "-c", src, "-o", obj])
    if jobs:
        if verbose:
            print(f"[build] compiling {len(jobs)} HIP translation unit(s) for gfx950", flush=True)
        with cf.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            list(ex.map(_run, jobs))
    if jobs or not os.path.exists(LIB_HIP):
        _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_HIP, *objs])
    return LIB_HIP


QUANT_PROBE_SRC = os.path.join(ROOT, "tests", "quant_probe", "quant_probe.hip")
LIB_QUANT_PROBE = os.path.join(os.path.dirname(QUANT_PROBE_SRC), "libsvc_quant_probe.so")


def build_quant_probe(force: bool = False) -> str:
    """TEST ONLY: csrc/quant_core.hpp's fused-kernel quantiser on a plain array (tests/test_gpu_transform_exact.py), a small library
    of its own with the product's flags -- libsvc_hip.so gains no symbol for it."""
    deps = [QUANT_PROBE_SRC] + _headers()
    if force or not _newer(LIB_QUANT_PROBE, deps):
        _run([_hipcc(), *HIPCC_FLAGS, "-shared", "-o", LIB_QUANT_PROBE, QUANT_PROBE_SRC])
    return LIB_QUANT_PROBE


HIPCC_HOST_SOURCES = [os.path.join("host", f) for f in ("stream_encoder.cpp", "stream_decoder.cpp", "clip_encoder.cpp", "wire_transcoder.cpp")]


def build_motion(force: bool = False) -> str:
    """The C++ layer above the C ABI: the reference's motion.hpp entry points (plain C++, g++) and the
    batched host-memory encoder (uses the HIP runtime for buffers, streams and events: hipcc, host only)."""
    srcs = [os.path.join(CSRC, s) for s in HOST_SOURCES]
    hip_srcs = [os.path.join(CSRC, s) for s in HIPCC_HOST_SOURCES]
    if force or not _newer(LIB_MOTION, srcs + hip_srcs + _headers() + [LIB_HIP]):
        cxx = shutil.which("g++") or "g++"
        objs = [os.path.join(OBJ, os.path.basename(src).replace(".cpp", ".o")) for src in hip_srcs]
        for src, obj in zip(hip_srcs, objs):
            _run([_hipcc(), "-std=c++17", "-O2", "-fPIC", "-Wall", f"-I{INCLUDE}", "-c", src, "-o", obj])
        rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "lib")
        _run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", f"-I{INCLUDE}", f"-I{os.path.join(INCLUDE, 'svc')}",
              "-o", LIB_MOTION, *srcs, *objs, f"-L{PKG}", "-lsvc_hip", f"-L{rocm_lib}", "-lamdhip64",
              "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{rocm_lib}"])
    return LIB_MOTION


DROPIN_SRC = os.path.join(ROOT, "tests", "dropin", "dropin_main.cpp")
REFERENCE_LIBS = os.environ.get("SVC_REFERENCE_DIR", "/root/reference") + "/libs"


# Host applications written against the public C++ headers only, one source each, all built by the same line:
DROPIN_APPS = [
    "stream_main",          # include/svc/stream_encoder.hpp
    "stream_levels_main",   # ... with the compact quantised-coefficient output (StreamEncoderConfig::compact): tests/test_gpu_levels.py
    "stream_budget_main",   # ... and with rate control (compact_budget, SetCompactBudget): tests/test_gpu_levels_budget.py
    "stream_entropy_main",  # ... and with the entropy-coded output, decoded again by svc::StreamDecoder: tests/test_gpu_entropy.py
    "stream_decode_main",   # svc::StreamDecoder: stream_levels_main's output -> display frames, tests/test_gpu_decode_levels.py
    "stream_reduced_main",  # svc::StreamDecoder with StreamDecoderConfig::reduce: display frames at 1/2, 1/4, 1/8 size, tests/test_gpu_decode_reduced.py
    "stream_layers_main",   # two layers: compact + enh_step, and svc::StreamDecoder::DecodeLayers on them: tests/test_gpu_stream_layers.py
    "stream_layers_reduced_main",  # DecodeLayers with StreamDecoderConfig::reduce on stream_layers_main's files: tests/test_gpu_decode_layers_reduced.py
    "stream_delta_main",    # svc::StreamDecoder::DecodeDelta: a delta stream (SVCQ or SVCE) -> display frames, tests/test_gpu_stream_delta.py
    "stream_delta_reduced_main",  # svc::StreamDecoder::DecodeDeltaReduced: a delta stream or its band -> display frames at 1/2, 1/4, 1/8 size, tests/test_gpu_stream_delta_reduced.py
    "stream_delta_encode_main",  # StreamEncoderConfig::delta: a raw clip -> the delta stream and its key flags, tests/test_gpu_stream_delta_encode.py
    "stream_delta_auto_main",  # StreamEncoderConfig::auto_key: a raw clip -> the delta stream with its key frames chosen by size, played by DecodeDelta: tests/test_gpu_stream_delta_auto.py
    "stream_delta_budget_main",  # StreamEncoderConfig::delta with compact_budget: a raw clip -> the delta stream with one ladder entry per group of frames, tests/test_gpu_stream_delta_budget.py
    "stream_delta_quality_main",  # StreamEncoderConfig::delta with compact_quality: a raw clip -> the delta stream at a PSNR held per group of frames, tests/test_gpu_stream_delta_quality.py
    "stream_temporal_main",  # StreamEncoderConfig::temporal_period: a raw clip -> the delta stream with temporal layers, thinned and played by DecodeDeltaTemporal: tests/test_gpu_stream_temporal.py
    "stream_temporal_reduced_main",  # svc::StreamDecoder::DecodeDeltaTemporalReduced: a temporal-layer delta stream or its band -> display frames at 1/2, 1/4, 1/8 size, tests/test_gpu_stream_temporal_reduced.py
    "wire_decode_main",     # svc::StreamDecoder::DecodeWire: a reference stream on stdin -> display frames, tests/test_gpu_decode_records.py
    "wire_transcode_main",  # svc::WireTranscoder: a reference stream on stdin -> the compact stream, and back: tests/test_gpu_wire_transcode.py
    "stream_fuzz",          # the encoder at random against itself (batch sizes, depths, entry points, reuse): tests/test_gpu_stream.py
]


def build_dropin(force: bool = False) -> List[str]:
    """A caller written against the reference's motion.hpp only, linked to libsvc_motion.so:
    once with the reference's OWN header (where /root/reference exists; the binary travels
    to the GPU box), once with include/svc/motion.hpp."""
    cxx = shutil.which("g++") or "g++"
    out = []
    variants = [("dropin_own_hdr", os.path.join(INCLUDE, "svc"), [])]
    if os.path.exists(os.path.join(REFERENCE_LIBS, "motion.hpp")):
        variants.append(("dropin_ref_hdr", REFERENCE_LIBS, []))
        variants.append(("dropin_ref_hdr_sse2", REFERENCE_LIBS, ["-DDROPIN_USE_SSE2_ENTRY"]))
    for name, inc, extra in variants:
        exe = os.path.join(os.path.dirname(DROPIN_SRC), name)
        if force or not _newer(exe, [DROPIN_SRC, LIB_MOTION]):
            _run([cxx, "-std=c++17", "-O2", "-msse2", f"-I{inc}", *extra, "-o", exe, DROPIN_SRC, f"-L{PKG}",
                  "-lsvc_motion", "-lsvc_hip", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../scalable_video_codec_amd"])
        out.append(exe)
    for name in DROPIN_APPS:
        exe = os.path.join(os.path.dirname(DROPIN_SRC), name)
        src = exe + ".cpp"
        if force or not _newer(exe, [src, LIB_MOTION]):  # (the library is newer than every header)
            _run([cxx, "-std=c++17", "-O2", f"-I{INCLUDE}", "-o", exe, src, f"-L{PKG}", "-lsvc_motion", "-lsvc_hip",
                  f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../scalable_video_codec_amd", "-Wl,--allow-shlib-undefined"])
        out.append(exe)
    return out


COMPAT = os.path.join(ROOT, "compat")
LIB_COMPAT = os.path.join(PKG, "libsvc_opencv_compat.so")


def build_compat(force: bool = False) -> str:
    """compat/opencv2: the slice of the OpenCV API the reference's encoder uses, every arithmetic call forwarding to
    include/svc_hip.h (a product-side adapter -- never an oracle).  Plain C++ on top of the C ABI."""
    srcs = [os.path.join(COMPAT, "src", f) for f in ("core.cpp", "imgproc.cpp", "videoio.cpp")]
    hdrs = [os.path.join(COMPAT, "src", "internal.hpp")] + _headers() + \
        [os.path.join(COMPAT, "opencv2", f) for f in ("core.hpp", "imgproc.hpp", "videoio.hpp", os.path.join("core", "mat.hpp"))]
    if force or not _newer(LIB_COMPAT, srcs + hdrs + [LIB_HIP]):
        cxx = shutil.which("g++") or "g++"
        _run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", f"-I{COMPAT}", f"-I{INCLUDE}", f"-I{CSRC}", "-o", LIB_COMPAT,
              *srcs, f"-L{PKG}", "-lsvc_hip", "-Wl,-rpath,$ORIGIN"])
    return LIB_COMPAT


REFERENCE_APPS = os.environ.get("SVC_REFERENCE_DIR", "/root/reference") + "/apps"


def reference_encoder_command(exe: str, sse2: bool, extra_sources: List[str] = ()) -> List[str]:
    """THE build line of INTEGRATION.md section 6: the reference's own apps/encoder.cpp + libs/encoder.cpp + libs/cli.cpp,
    compiled where they lie (never copied, never edited), against compat/opencv2 instead of OpenCV, with this repo's
    ThreadGuard in place of the reference's thread.cpp (which does not compile), linked to the three product libraries."""
    cxx = shutil.which("g++") or "g++"
    return [cxx, "-std=c++17", "-O2", "-DNDEBUG", "-msse2", *(["-DSVC_MOTION_SSE2"] if sse2 else []),
            f"-I{COMPAT}", f"-I{REFERENCE_LIBS}", "-o", exe,
            os.path.join(REFERENCE_APPS, "encoder.cpp"), os.path.join(REFERENCE_LIBS, "encoder.cpp"),
            os.path.join(REFERENCE_LIBS, "cli.cpp"), os.path.join(COMPAT, "src", "thread_guard.cpp"), *extra_sources,
            f"-L{PKG}", "-lsvc_opencv_compat", "-lsvc_motion", "-lsvc_hip", "-pthread",
            f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../scalable_video_codec_amd"]


def svc_encoder_app_command(exe: str, sse2: bool = True, extra_sources: List[str] = ()) -> List[str]:
    """INTEGRATION.md section 3, second build line: the reference's unchanged apps/encoder.cpp + libs/cli.cpp with THIS repo's
    implementation of the reference's class Encoder (csrc/host/encoder_hip.cpp, compiled against the reference's own encoder.hpp)
    in place of libs/encoder.cpp -- the batched GPU form of the same application."""
    cxx = shutil.which("g++") or "g++"
    return [cxx, "-std=c++17", "-O2", "-DNDEBUG", "-msse2", *(["-DSVC_MOTION_SSE2"] if sse2 else []), f"-I{COMPAT}", f"-I{REFERENCE_LIBS}",
            f"-I{INCLUDE}", "-o", exe, os.path.join(REFERENCE_APPS, "encoder.cpp"), os.path.join(REFERENCE_LIBS, "cli.cpp"),
            os.path.join(CSRC, "host", "encoder_hip.cpp"), os.path.join(COMPAT, "src", "thread_guard.cpp"), *extra_sources,
            f"-L{PKG}", "-lsvc_opencv_compat", "-lsvc_motion", "-lsvc_hip", "-pthread",
            f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../scalable_video_codec_amd"]


def build_reference_encoder(force: bool = False) -> List[str]:
    """tests/dropin/ref_encoder_{sse2,generic}: the reference's unchanged encoder application on the HIP path,
    built where /root/reference exists; the binaries travel to the GPU box like the other drop-in callers.  The only extra
    object is tests/dropin/ransac_seed.cpp, a TEST seam (it seeds the wrapper's RANSAC engine before main() so that the
    output stream is repeatable; the reference seeds from std::random_device)."""
    if not os.path.exists(os.path.join(REFERENCE_APPS, "encoder.cpp")):
        return []
    here = os.path.dirname(DROPIN_SRC)
    seed_src = os.path.join(here, "ransac_seed.cpp")
    deps = [LIB_COMPAT, LIB_MOTION, seed_src, os.path.join(COMPAT, "src", "thread_guard.cpp")] + \
        [os.path.join(COMPAT, "opencv2", f) for f in ("core.hpp", "imgproc.hpp", "videoio.hpp", os.path.join("core", "mat.hpp"))]
    out = []
    for name, sse2 in (("ref_encoder_sse2", True), ("ref_encoder_generic", False)):
        exe = os.path.join(here, name)
        if force or not _newer(exe, deps):
            _run(reference_encoder_command(exe, sse2, [seed_src]))
        out.append(exe)
    # the reference's unchanged apps/encoder.cpp on the BATCHED Encoder (csrc/host/encoder_hip.cpp: class Encoder of the reference's own
    # encoder.hpp implemented on svc::StreamEncoder) instead of the reference's libs/encoder.cpp
    enc_src = os.path.join(CSRC, "host", "encoder_hip.cpp")
    seed2 = os.path.join(here, "encoder_seed.cpp")
    for name, sse2 in (("ref_app_svc_encoder", True), ("ref_app_svc_encoder_generic", False)):
        exe = os.path.join(here, name)
        if force or not _newer(exe, [enc_src, seed2, LIB_COMPAT, LIB_MOTION, os.path.join(INCLUDE, "svc", "stream_encoder.hpp")]):
            _run(svc_encoder_app_command(exe, sse2, [seed2]))
        out.append(exe)
    # the libstdc++ engine + distribution the C++ RANSAC wrapper draws with, for tests that mirror its draws
    exe = os.path.join(here, "ransac_draws")
    src = os.path.join(here, "ransac_draws.cpp")
    if force or not _newer(exe, [src]):
        _run([shutil.which("g++") or "g++", "-std=c++17", "-O2", "-o", exe, src])
    out.append(exe)
    return out


def build_all(force: bool = False, verbose: bool = False) -> None:
    build_hip(force, verbose)
    build_quant_probe(force)
    build_motion(force)
    build_compat(force)
    build_dropin(force)
    build_reference_encoder(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
    print(LIB_HIP)
    print(LIB_MOTION)
