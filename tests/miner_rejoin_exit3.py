"""A re-spawned miner rank that dies before it is ready (tests/test_miner_rejoin.py): exits 3 at once."""
import sys

sys.exit(3)
