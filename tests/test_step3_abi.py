"""CPU-side checks of the device-resident 3-D step's C ABI: the two structs of pl3_resident_step as the library compiled them
against their ctypes mirrors, and the option that selects the step."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_step3_struct_layouts_match_header():
    from pylamp_amd import _lib
    lay = (C.c_size_t * 8)()
    assert _lib.load().pl3_abi_layout(lay) == 0
    SC, SR = _lib.Step3Config, _lib.Step3Report
    assert list(lay) == [C.sizeof(SC), C.sizeof(SR), SC.bcheatvals.offset, SC.grav.offset, SC.inject_seed.offset, SR.heat.offset,
                         SR.ntrac.offset, SR.ms_total.offset]
    assert SR.heat.offset - SR.stokes.offset == C.sizeof(_lib.SolveStats)


def test_step3_struct_fields_follow_the_header_order():
    from pylamp_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pylamp_hip.h")).read()
    for name, mirror in (("pl3_step_config", _lib.Step3Config), ("pl3_step_report", _lib.Step3Report)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[.*\]", "", v).strip() for v in decl.split(None, 1)[1].split(",")]
        assert fields == [f for f, _ in mirror._fields_], name


def test_step3_symbols_are_exported_and_resident_is_an_option():
    from pylamp_amd import _lib, pylamp3d as P3
    lib = _lib.load()
    for n in ("pl3_resident_step", "pl3_get_field", "pl3_transfer_stats", "pl3_advection_velocity", "pl3_abi_layout"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert P3.Options3().resident is False
    assert P3.Options3(resident=True).resident is True
