"""sgm_create allocates what it allocated: sgm_device_bytes of one small handle
per allocation path (tests/device_bytes_recipe.py) equals the value recorded
from the commit before sgm_create was rebuilt around plan_handle
(tests/golden/device_bytes.json, tests/golden/make_device_bytes_golden.py)."""
from __future__ import annotations

import json
import os

import pytest

import device_bytes_recipe as recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "device_bytes.json")))


def test_every_case_is_recorded():
    assert set(GOLDEN) == set(recipe.CASES)
    assert all(isinstance(v, int) and v > 0 for v in GOLDEN.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(recipe.CASES))
def test_device_bytes_as_recorded(name):
    assert recipe.measure(name) == GOLDEN[name]
