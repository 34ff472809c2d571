"""tests/test_emu_brotli_rec_par_api.py's legs through the library on the device."""
import pytest

import brotli_rec_api as A

pytestmark = pytest.mark.gpu


def test_api_legs():
    A.check_legs("gpu")
