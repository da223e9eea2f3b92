"""CPU: the C ABI of the fused CRC32 + CRC32C call (aws_crt_amd_crc32_dual_strided): its argument
checks, which come before any device work, the loud failure without a device, and the fused kernel's
private segment size read from the code object's metadata (no scratch, no spilled arguments)."""
import ctypes
import glob
import shutil
import subprocess

from tests.libpaths import ENGINE as LIB, load_engine

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
ERR_NO_DEVICE, ERR_INVALID_ARG = -1, -2


def dual(L):
    f = L.aws_crt_amd_crc32_dual_strided
    f.restype, f.argtypes = ctypes.c_int, [VP, SZ, SZ, SZ, VP, VP, VP]
    L.aws_crt_amd_last_error.restype = ctypes.c_char_p
    return f


def test_dual_symbols_exported():
    L = load_engine()
    dual(L)
    L.aws_crt_amd_crc32_dual_fused_launches.restype = ctypes.c_ulonglong
    assert L.aws_crt_amd_crc32_dual_fused_launches() >= 0


def test_dual_argument_checks():
    """count 0 is a no-op; a null d_out, a null base with len > 0 and a stride that is no multiple of 16
    (count > 1) are AWS_CRT_AMD_ERR_INVALID_ARG -- all before any device work"""
    L = load_engine()
    f = dual(L)
    assert f(None, 0, 0, 0, None, None, None) == 0
    assert f(VP(0x1000), 16, 16, 0, None, VP(0x2000), None) == 0
    assert f(VP(0x1000), 16, 16, 1, None, None, None) == ERR_INVALID_ARG
    assert b"null buffer" in L.aws_crt_amd_last_error()
    assert f(None, 16, 16, 1, None, VP(0x2000), None) == ERR_INVALID_ARG
    assert b"null buffer" in L.aws_crt_amd_last_error()
    assert f(VP(0x1000), 24, 16, 2, None, VP(0x2000), None) == ERR_INVALID_ARG
    assert b"stride % 16" in L.aws_crt_amd_last_error()


def test_dual_no_device_fails_loudly():
    """without a device a well-formed call returns AWS_CRT_AMD_ERR_NO_DEVICE (device addresses cannot
    be read by the host path); with a device the no-op forms above are all this test can ask"""
    L = load_engine()
    f = dual(L)
    if L.aws_crt_amd_device_count() == 0:
        assert f(VP(0x1000), 16, 16, 1, None, VP(0x2000), None) == ERR_NO_DEVICE
        assert b"no HIP device" in L.aws_crt_amd_last_error()
        # a stride that count == 1 makes irrelevant is not an argument error
        assert f(VP(0x1000), 24, 16, 1, None, VP(0x2000), None) == ERR_NO_DEVICE
        # len 0 with a null base is well formed (the results are the seeds)
        assert f(None, 0, 0, 3, None, VP(0x2000), None) == ERR_NO_DEVICE
    else:
        assert f(None, 0, 0, 0, None, None, None) == 0


def test_dual_kernels_keep_their_arguments_out_of_scratch(tmp_path):
    """crc32_dual_stream_kernel and its finish pass hold a private segment of at most 32 bytes: the bar
    tests/test_abi.py sets for the existing scans"""
    llvm = "/opt/rocm/lib/llvm/bin"
    lib = shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", str(lib)], cwd=tmp_path, check=True, capture_output=True)
    cos = glob.glob(str(tmp_path / "lib.so.*gfx950"))
    assert cos, "no gfx950 code object in the library"
    seen = {}
    for co in cos:
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        name = None
        for line in notes.splitlines():
            line = line.strip()
            if line.startswith(".name:"):
                name = line.split(":", 1)[1].strip()
            elif line.startswith(".private_segment_fixed_size:") and name and "DualParams" in name:
                seen[name] = int(line.split(":", 1)[1])
    assert any("crc32_dual_stream_kernel" in n for n in seen) and any("crc32_dual_finish_kernel" in n for n in seen), seen
    for name, size in seen.items():
        assert size <= 32, (name, size)
