"""CPU suite: what tests/test_gpu_persistent_rows.py relies on before anything runs on a GPU.  That file imports; its two
selections have the properties its tests name (a 64-marker chromosome with 63 first loci, chromosomes with one selected
marker and with none); the descent oracle leaves no (individual, chromosome) of the four fixtures out and meets, on its own,
every condition the GPU tests set; so does the pair oracle, on the smallest fixture and both selections (the fixtures of 158
markers take the pair oracle a quarter of a minute each: the GPU suite holds them to the same conditions where it makes
them)."""
import pytest

import test_gpu_persistent_rows as rows_suite
from test_gpu_persistent_modes import FIXTURES, fixture


@pytest.mark.parametrize("name", FIXTURES)
def test_selections(name):
    sels = rows_suite.check_selections(fixture(name))
    assert {"sel_all", "sel_sparse"} <= set(sels) <= {"sel_all", "sel_sparse", "sel_thin"}


@pytest.mark.parametrize("name", FIXTURES)
def test_descent_reference_alone(name):
    rows_suite.check_reference_alone(fixture(name), modes=("descent",))


def test_pair_reference_alone():
    rows_suite.check_reference_alone(fixture("tied_mixed"), modes=("pairs",))
