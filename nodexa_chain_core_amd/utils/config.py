"""Argument / config-file handling with the reference's ArgsManager semantics.

Parity: ArgsManager (src/util.h:225), ParseParameters (src/util.cpp:407) —
`-name`, `-name=value`, `--name=value`, `-noname` (negation), repeated
options become lists; ReadConfigFile (src/util.cpp:631) — `name=value`
lines, `#` comments, `[main]/[test]/[regtest]` sections that apply only to
that network; command line wins over the file; SoftSetArg / ForceSetArg;
network selection from -regtest / -testnet (SelectParams).

New engine flags: -gpus=0,1,.. -kawpowactivationtime= -equihash
-gpuintensity= -dagcache= -gpufailrate= -dropshare= -strictheight -dbformat=leveldb|journal
-kawpowjit=wait|auto|off (default wait): what the KawPow GPU miner does while a ProgPoW period's
compiled kernel does not exist yet: wait for the compile, mine on the period-agnostic kernel until
it is there (auto), or never compile (off). Any other value is an init error.

-minerrejoin=<seconds> (default 0 = never): a GPU rank of the node's miner world that was evicted
(-minermaxfailures) or hung (-minerwatchdog) is started again that long after its process ended and
taken back into the world. -minerrejoinmax=<n> (default 3) such endings within
-minerrejoinwindow=<seconds> (default 600) leave the GPU evicted. Not in torchrun worlds.

-dagcheck=0|1 (default 1; NODEXA_DAG_CHECK): the KawPow GPU miner checks every DAG it builds (each
received shard against its owner's digest, a sampled audit against the light cache) and seals it
with per-chunk digests. -dagscrub=<seconds> (default 0 = off; NODEXA_DAG_SCRUB_S): while mining,
digest the resident DAG that often, compare with the seal and repair damaged chunks from the light
cache; needs -dagcheck=1. The flags reach every rank of the miner world through those variables.

-maxconnections=<n>: maintain at most <n> connections to peers in total (default 125), as in the
reference: up to min(8, n) of them outbound, and n less the outbound slots and one more for
inbound peers; at that limit a new inbound peer takes the place of an evictable one or is refused.

-scriptcache=0|1 (default 0; the reference has this cache always on): the script-execution cache. A
transaction that passes mempool acceptance is run once more under the block's script flags and
remembered by (witness hash, flags); the block that confirms it then runs none of its scripts, on
the host path and in the GPU batch (-gpusigs, -gpusighash, -gpumultisig, -gpusigwindow) alike. The
cache takes half of -maxsigcachesize (default 32 MiB, so 16 MiB), the reference's split; the
signature cache keeps the whole figure here. -maxsigcachesize=0 keeps nothing in either cache.

Stratum server of the node (miner/stratum_server.py; needs -miningaddress, KawPow only):
-stratumport=<port> (off without it), -stratumbind=<addr> (default 127.0.0.1), -stratumsharebits=<n>
(share target 2^(256-n) - 1 as -minertargetbits; the effective target is the easier of it and the
block target), -stratumpassword=<pw> (mining.authorize must present it), -stratummaxconn=<n>
(default 64; further connections are refused), -stratumvardiff=<shares per minute> (default 0 =
off: a share target per connection, from -stratumsharebits upwards, steered to that rate; needs
-stratumsharebits above 0), -stratumgpuverify=0|1 (default 0: with 1 and a GPU the server builds
the DAG of the served epoch itself when the miner has none there, and the next epoch's 120 blocks
ahead, so that shares are checked on the GPU; -dagcheck applies), -stratumbantime=<seconds>
(default 0 = off: an address closed for a wrong mix 3 times within 10 minutes is refused that
long). nodexa-miner: -stratum=host:port (repeatable, tried
in order), -stratumuser=, -stratumpass= (default x).
"""
from __future__ import annotations

import os
import threading

DEFAULT_CONF = "nodexa.conf"
NETWORKS = ("main", "test", "regtest")
KAWPOW_JIT_MODES = ("wait", "auto", "off")  # ops/jit.JIT_MODES (kept apart: no native import here)


def kawpow_jit_mode(args: "ArgsManager") -> str:
    """-kawpowjit=wait|auto|off, validated (ValueError with the init-error text otherwise)."""
    mode = args.get("kawpowjit", "wait") or "wait"
    if mode not in KAWPOW_JIT_MODES:
        raise ValueError(f"Error: invalid -kawpowjit={mode} (expected {', '.join(KAWPOW_JIT_MODES[:-1])} "
                         f"or {KAWPOW_JIT_MODES[-1]})")
    return mode


def miner_rejoin_args(args: "ArgsManager") -> tuple[float, int, float]:
    """(-minerrejoin, -minerrejoinmax, -minerrejoinwindow), validated (ValueError with the init-error
    text otherwise)."""
    try:
        delay = float(args.get("minerrejoin", "0") or 0)
        n = int(args.get("minerrejoinmax", "3") or 3)
        window = float(args.get("minerrejoinwindow", "600") or 600)
    except ValueError:
        raise ValueError("Error: -minerrejoin, -minerrejoinmax and -minerrejoinwindow take numbers") from None
    if delay < 0 or n < 1 or window <= 0:
        raise ValueError("Error: -minerrejoin must not be negative, -minerrejoinmax at least 1 and "
                         "-minerrejoinwindow positive")
    return delay, n, window


def dag_check_args(args: "ArgsManager") -> tuple[bool | None, float | None]:
    """(-dagcheck, -dagscrub), validated (ValueError with the init-error text otherwise); None for a
    flag that was not given (the environment's NODEXA_DAG_CHECK / NODEXA_DAG_SCRUB_S then decide)."""
    check = args.get("dagcheck")
    if check is not None and check not in ("0", "1", ""):
        raise ValueError(f"Error: invalid -dagcheck={check} (expected 0 or 1)")
    scrub = args.get("dagscrub")
    try:
        scrub_s = None if scrub is None else float(scrub or 0)
    except ValueError:
        raise ValueError("Error: -dagscrub takes a number of seconds") from None
    if scrub_s is not None and scrub_s < 0:
        raise ValueError("Error: -dagscrub must not be negative")
    return (None if check is None else check != "0"), scrub_s


class ArgsManager:
    def __init__(self) -> None:
        self._lock = threading.RLock()
        self._cli: dict[str, list[str]] = {}
        self._conf: dict[str, list[str]] = {}
        self._forced: dict[str, list[str]] = {}
        self._network = "main"

    # ------------------------------------------------------------ parsing
    @staticmethod
    def _norm(key: str) -> tuple[str, bool]:
        key = key.lstrip("-")
        if key.startswith("no") and len(key) > 2 and not key.startswith("nonce"):
            return key[2:], True
        return key, False

    def parse_parameters(self, argv: list[str]) -> list[str]:
        """Parse `-flag[=value]` options; returns the positional remainder."""
        rest: list[str] = []
        with self._lock:
            self._cli.clear()
            for i, a in enumerate(argv):
                if not a.startswith("-") or a in ("-", "--"):
                    rest.extend(argv[i:])
                    break
                name, _, value = a.partition("=")
                key, neg = self._norm(name)
                if neg:
                    value = "0" if value in ("", "1") else ("1" if value == "0" else value)
                elif "=" not in a:
                    value = "1"
                self._cli.setdefault(key, []).append(value)
            self._network = self._select_network()
        return rest

    def read_config_file(self, path: str) -> None:
        if not os.path.exists(path):
            return
        section = None
        with self._lock, open(path) as f:
            for raw in f:
                line = raw.split("#", 1)[0].strip()
                if not line:
                    continue
                if line.startswith("[") and line.endswith("]"):
                    section = line[1:-1].strip()
                    continue
                name, _, value = line.partition("=")
                key, neg = self._norm(name.strip())
                value = value.strip()
                if neg:
                    value = "0"
                elif "=" not in line:
                    value = "1"
                full = key if section is None else f"{section}.{key}"
                self._conf.setdefault(full, []).append(value)
            self._network = self._select_network()

    def _select_network(self) -> str:
        reg = self._raw_bool("regtest")
        test = self._raw_bool("testnet")
        if reg and test:
            raise ValueError("Invalid combination of -regtest and -testnet.")
        return "regtest" if reg else ("test" if test else "main")

    # ------------------------------------------------------------ getters
    def _values(self, key: str) -> list[str] | None:
        key = key.lstrip("-")
        with self._lock:
            if key in self._forced:
                return self._forced[key]
            if key in self._cli:
                return self._cli[key]
            sec = f"{self._network}.{key}"
            if sec in self._conf:
                return self._conf[sec]
            if key in self._conf:
                return self._conf[key]
        return None

    def _raw_bool(self, key: str) -> bool:
        v = self._cli.get(key) or self._conf.get(key)
        return bool(v) and _truthy(v[-1])

    @property
    def network(self) -> str:
        return self._network

    def is_set(self, key: str) -> bool:
        return self._values(key) is not None

    def get(self, key: str, default: str | None = None) -> str | None:
        v = self._values(key)
        return v[-1] if v else default

    def get_int(self, key: str, default: int) -> int:
        v = self.get(key)
        try:
            return int(v) if v is not None else default
        except ValueError:
            return default

    def get_bool(self, key: str, default: bool = False) -> bool:
        v = self.get(key)
        return default if v is None else _truthy(v)

    def get_list(self, key: str) -> list[str]:
        return list(self._values(key) or [])

    def soft_set(self, key: str, value: str) -> bool:
        """Set only if the user did not (SoftSetArg)."""
        if self.is_set(key):
            return False
        self.force_set(key, value)
        return True

    def force_set(self, key: str, value: str) -> None:
        with self._lock:
            self._forced[key.lstrip("-")] = [value]

    def data_dir(self) -> str:
        base = os.path.expanduser(self.get("datadir", os.path.join("~", ".nodexa")))
        path = base if self._network == "main" else os.path.join(base, "testnet7" if self._network == "test"
                                                                 else "regtest")
        os.makedirs(path, exist_ok=True)
        return path


def _truthy(v: str) -> bool:
    v = v.strip().lower()
    if v in ("", "1", "true", "yes", "on"):
        return True
    if v in ("0", "false", "no", "off"):
        return False
    try:
        return int(v) != 0
    except ValueError:
        return True


def gpu_list(args: ArgsManager) -> list[int]:
    """`-gpus=0,1,3` -> [0, 1, 3]; `-gpus=all` -> every visible device; unset -> []."""
    v = args.get("gpus")
    if v is None or v.strip().lower() in ("", "none", "off"):
        return []
    if v == "all":
        import torch

        return list(range(torch.cuda.device_count()))
    return [int(x) for x in v.split(",") if x.strip() != ""]


g_args = ArgsManager()
