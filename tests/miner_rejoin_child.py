"""A dummy follower for the supervisor tests (tests/test_miner_rejoin.py): writes the environment the
supervisor gave it to argv[1], then exits with argv[2], or sleeps when argv[2] is "sleep"."""
import json
import os
import sys
import time

with open(sys.argv[1], "w") as f:
    json.dump({k: os.environ.get(k) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NODEXA_MINER_DEVICE",
                                               "NODEXA_MINER_LIFE", "NODEXA_MINER_JOIN_MEMBERSHIP", "EXTRA")}, f)
if sys.argv[2] == "sleep":
    time.sleep(600)
sys.exit(int(sys.argv[2]))
