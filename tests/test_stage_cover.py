"""What the cases of tests/test_gpu_refidx.py, tests/test_gpu_stages_1080p.py
and the tie test of tests/test_gpu_seed.py cover is asserted on the CPU
references alone.  Those functions live beside their cases, in modules marked
`gpu`; they need no device, so the CPU suite runs them from here as well."""
from test_gpu_refidx import test_the_partition_leaves_use_every_reference  # noqa: F401
from test_gpu_refidx import test_the_refidx_cases_cover_what_they_should  # noqa: F401
from test_gpu_seed import test_the_stripe_rows_tie  # noqa: F401
from test_gpu_stages_1080p import test_the_cut_lies_on_the_minimum_of_odd_cut_rows  # noqa: F401
from test_gpu_stages_1080p import test_the_odd_cut_rows_are_what_the_tables_say  # noqa: F401
from test_gpu_stages_1080p import test_the_wide_search_meets_the_cut_on_odd_cut_rows  # noqa: F401
