"""CPU-side checks of the strain-field additions to the C ABI and to Options3: the header declares the entry points, the library exports
them, _lib binds them, and Simulation3 rejects shear heating without the heat solve before it touches a device."""
import os
import re

import pytest

from conftest import ROOT

NEW = ("pl3_stokes_strain_fields", "pl3_step_set_shear_heating", "pl3_step_shear_heating", "pl3_step_set_strain_fields",
       "pl3_step_dissipation_total")


def test_symbols_declared_exported_and_bound():
    from pylamp_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pylamp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(pl3_ctx\* ctx" % n, code), "not declared: " + n
        assert hasattr(lib, n), "missing export " + n
        assert n in _lib.SIGNATURES, "no ctypes signature for " + n
    assert len(_lib.SIGNATURES["pl3_stokes_strain_fields"][1]) == 8
    # the definition is written down at the entry point
    doc = re.sub(r"\s*\n \*\s*", " ", txt)
    for word in ("eps_DE = 1/2 (g_DE + g_ED)", "control-volume weighted mean", "pl3_set_comm attached", "one IEEE addition per node"):
        assert word in doc, word


def test_options_and_rejection_by_name():
    from pylamp_amd import pylamp3d as P3
    o = P3.Options3()
    assert o.shear_heating is False and o.strain_fields is False
    assert P3.Options3(shear_heating=True, strain_fields=True).shear_heating is True
    with pytest.raises(Exception, match="Options3.shear_heating = True needs the heat solve, Options3.do_heatdiff = True"):
        P3.Simulation3([9, 9, 9], [1.0, 1.0, 1.0], options=P3.Options3(shear_heating=True, do_heatdiff=False))
    assert P3.STRAIN_FIELDS == ("strainrate", "stress", "dissipation")
