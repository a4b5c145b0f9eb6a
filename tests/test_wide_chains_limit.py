"""CPU: the chain limit of a rank (HTM_MAX_CHAINS = 64) is the header's, and the Python layer refuses more chains before it
touches a device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_header_and_python_agree_on_the_chain_limit():
    from hypotremormcmc_amd import _lib

    src = open(os.path.join(ROOT, "include", "htm_hip.h")).read()
    m = re.search(r"^#define\s+HTM_MAX_CHAINS\s+(\d+)\s*$", src, flags=re.M)
    assert m and int(m.group(1)) == 64
    assert _lib.HTM_MAX_CHAINS == 64


def test_chain_set_refuses_65_chains_without_a_device():
    from hypotremormcmc_amd.chains import ChainSet

    with pytest.raises(ValueError, match=r"\b64\b"):
        ChainSet(None, [None] * 65, np.ones(65), (1, 2, 3, 4))
