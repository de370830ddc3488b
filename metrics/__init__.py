"""Import-by-name drop-in for the reference's `metrics` package (see models/__init__.py): with this repository's root ahead of the
reference's on `sys.path`, `from metrics.stats_utils import ...` in the reference's compute_stats.py lands on hover_net_amd.metrics."""
