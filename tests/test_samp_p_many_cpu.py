"""No-GPU checks of samp_p_dev_many (include/psf_mi355x.h): the three entry points are exported, a NULL handle is refused before anything touches a device,
and the Rust shim's extern block carries their prototypes."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("psfp_samp_p_dev_many", "psfgpv_samp_p_dev_many", "psfring_samp_p_dev_many")


def test_the_three_entry_points_are_exported():
    lib = os.path.join(ROOT, "tools_amd", "lib", "libpsf_mi355x.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in syms.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name


def test_a_null_handle_is_a_parameter_error():
    from tools_amd import _ffi
    lib = _ffi.lib()
    seeds = (C.c_uint64 * 2)(1, 2)
    firsts = (C.c_uint64 * 2)(0, 10)
    for name in NAMES:
        f = getattr(lib, name)
        assert f(None, C.c_size_t(2), seeds, firsts, C.c_size_t(4), C.c_void_p(16), C.c_void_p(16), None) == _ffi.ERR_PARAM, name
        assert f(None, C.c_size_t(0), None, None, C.c_size_t(4), None, None, None) == _ffi.ERR_PARAM, name


def test_the_shim_declares_the_prototypes():
    with open(os.path.join(ROOT, "shim", "src", "ffi.rs")) as fh:
        ffi = fh.read()
    assert "pub fn psfp_samp_p_dev_many(arg0: *mut psfp_handle, count: usize, seeds: *const u64, first_indices: *const u64, B: usize, d_u: *const u64, d_e: *mut i64, stream: *mut c_void) -> c_int;" in ffi
    for name in NAMES[1:]:
        assert f"pub fn {name}(" in ffi, name
