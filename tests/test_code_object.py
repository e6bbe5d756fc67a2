"""The shipped gfx950 code objects against the store-data hazard of wide stores (tools/check_store_hazard.py; DESIGN.md, "A
store-data hazard the ISA manual says does not exist").  CPU only: the library is disassembled, not run.

binarise.hip's tile stores keep the buffer store's scalar offset field 0 so that the compiler pads the slot behind them; with an
SGPR there it pads nothing and gfx950 corrupted mask words from the 16th frame of a batch on.  Whether the field stays 0 is the
compiler's choice, so it is checked in the binary."""
import os
import sys

import helpers as H

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import check_store_hazard as CSH  # noqa: E402

LIB = os.path.join(H.PKG, "lib", "libocvar_hip.so")


def test_checker_flags_an_sgpr_soffset_on_a_buffer_store():
    r = CSH.check_listing("""
0000000000003a00 <binarise_frames_kernel>:
	buffer_store_dwordx4 v[64:67], v40, s[28:31], s4 offen nt  // 000000003A54: E07E1000 04074028
	s_waitcnt lgkmcnt(0)
	buffer_store_dwordx3 v[68:70], off, s[28:31], 0 offset:16
	buffer_store_dword v1, v41, s[28:31], s5 offen
""")
    assert r.stores == 2
    assert len(r.failures) == 1 and r.failures[0].startswith("(a) soffset 's4'") and "binarise_frames_kernel" in r.failures[0]


def test_checker_flags_a_valu_write_of_store_data_in_the_next_slot():
    r = CSH.check_listing("""
	global_store_dwordx4 v[10:11], v[6:9], off offset:16
	v_mov_b32_e32 v9, -1
	buffer_store_dwordx4 v[20:23], v4, s[24:27], 0 offen nt
	v_add_u32_e32 v20, 1, v20
	scratch_store_dwordx4 off, a[0:3], s32
	v_accvgpr_write_b32 a2, v1
	buffer_store_dwordx4 v[30:33], v5, s[24:27], 0 offen nt
	s_nop 1
	v_mov_b32_e32 v30, 0
""")
    assert r.stores == 4
    assert [f.split(": ", 1)[1].split()[0] for f in r.failures] == ["global_store_dwordx4", "buffer_store_dwordx4", "scratch_store_dwordx4"]
    assert all(f.startswith("(b)") for f in r.failures)


def test_checker_ignores_address_registers_and_reports_non_valu_writes():
    r = CSH.check_listing("""
	global_store_dwordx4 v[10:11], v[6:9], off offset:16
	v_mov_b32_e32 v10, -1
	flat_store_dwordx3 v[2:3], v[4:6]
	v_mov_b32_e32 v3, 0
	buffer_store_dwordx4 v[34:37], v4, s[24:27], 0 offen nt
	scratch_load_dword v37, off, off
	global_store_dwordx3 v[8:9], v[2:4], off offset:136
	s_waitcnt vmcnt(0)
	global_load_dword v3, v[14:15], off offset:20
""")
    assert r.stores == 4 and r.failures == []
    assert len(r.notes) == 2 and all(n.startswith("(c)") for n in r.notes)
    assert "scratch_load_dword v37" in r.notes[0] and "global_load_dword v3" in r.notes[1]


def test_shipped_library_has_no_store_data_hazard():
    H._build(LIB, "lib/libocvar_hip.so", H.PKG)
    r = CSH.check_library(LIB)
    assert r.failures == [], "\n".join([CSH.compiler_version()] + r.failures)
    # the checker saw the binarise kernels' tile stores (a parser that found nothing would pass vacuously)
    for kernel in ("binarise_frames_kernel", "binarise_crops_kernel"):
        assert sum(n for k, n in r.per_mnemonic.items() if k.startswith("buffer_store_dwordx4 in ") and kernel in k) >= 2, kernel
    assert r.stores >= 50
