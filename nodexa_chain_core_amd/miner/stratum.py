"""Stratum for KawPow: the wire format, as pure functions (no sockets here).

Both ends in this tree (miner/stratum_client.py, miner/stratum_server.py) speak exactly this and
are tested against each other and against hand-written transcripts (tests/golden/stratum/). It
follows the KawPow Stratum dialect of pools and kawpowminer-style miners as far as we know it;
interoperation with third-party Stratum software is NOT verified.

Transport: TCP, one JSON object per "\\n"-terminated line, UTF-8. Requests carry `id`, `method`,
`params`. Responses carry `id`, `result`, `error`, where `error` is null or [code, message, null].
Server notifications carry "id": null.

  direction  method            params                                             result
  c->s       mining.subscribe  [agent, ...] (extra entries ignored)               [session_or_null, extranonce_hex]
  c->s       mining.authorize  [user, password]                                   true, or error 24
  s->c       mining.set_target [target]                                           -
  s->c       mining.notify     [job_id, header_hash, seed_hash, target,           -
                                clean_jobs, height, bits]
  c->s       mining.submit     [user, job_id, nonce, header_hash, mix_hash]       true, or an error

Field rules:
* `header_hash` and `mix_hash` are 64 hex digits in the byte order of `pprpcheader` and of
  `pprpcsb`'s mix argument (ProgPoW order).
* `nonce` is 16 hex digits, the 64-bit nonce as a number, as in `pprpcsb`.
* In `mining.submit` the three hex fields are sent with a `0x` prefix. The server accepts them with
  or without it.
* `seed_hash` is the ethash seed of `height`'s epoch, 64 hex digits.
* `target` is a 256-bit big-endian number in 64 hex digits, as getblocktemplate's `target`. A
  `target` in `mining.notify` replaces the last `mining.set_target`.
* `bits` is the compact nBits in 8 hex digits. It is informational.
* `extranonce_hex` is 0 to 12 hex digits, an even number of them. Those bytes are the most
  significant bytes of every nonce the connection may submit.
* Error codes: 20 other (bad params, wrong header hash for the job, nonce outside the extranonce,
  wrong mix), 21 job not found / stale, 22 duplicate share, 23 above the share target,
  24 unauthorized, 25 not subscribed.
* The client ignores unknown notifications. The server answers unknown methods with error 20.
* A line longer than 16 KiB, or one that is not a JSON object, closes the connection.

Nonce ranges: an extranonce of b bytes leaves `free = 64 - 8b` low bits. A work packet carries a
`rank_shift` s (miner/search.Work): rank r of the mining loop owns
[nonce_base + (r << s), nonce_base + ((r + 1) << s)), and `rank_shift_for` picks
s = free - ceil(log2(world_size)), at most 63 (an empty extranonce leaves 64 free bits).

Vardiff (the server's -stratumvardiff=<shares per minute>; `vardiff_next_bits`; this is the only
place the rule is written down). Every connection has share bits of its own, n, meaning the share
target 2^(256-n) - 1 (`share_target_for_bits`); it starts at lo_bits = -stratumsharebits, the easiest
target it can ever have, and never exceeds hi_bits = 255 (the job's block target still wins where it
is easier). A retarget looks at `shares`, the shares accepted since the connection's last retarget
(or its mining.authorize), and `elapsed_ms`, the time since then, in integers only:
    E = per_minute * elapsed_ms     (the wanted shares, times 60000)
    S = shares * 60000              (the shares there were, times the same)
    S >= 2E:  bits += min(4, floor(log2(S / E)))   too many shares: a harder target
    2S <= E:  bits -= min(4, floor(log2(E / S)))   too few: an easier one; shares == 0 counts as 4
    otherwise unchanged; then clamped to [lo_bits, hi_bits].
floor(log2(a / b)) is the largest k with a >= b * 2^k, found by shifting: no division, no float.
E == 0 (no time passed, or a rate of 0) measures nothing and leaves the bits as they are. One step
changes the target by at most 2^4, and inside (1/2, 2) of the wanted rate nothing moves, so a
connection near the wanted rate is left alone. When the rule runs is the server's business
(miner/stratum_server.py): only together with a job, so that a new target always travels as
mining.set_target in front of a mining.notify.
"""
from __future__ import annotations

import json
from dataclasses import dataclass

MAX_LINE = 16 * 1024
MAX_EXTRANONCE_DIGITS = 12

ERR_OTHER, ERR_STALE, ERR_DUPLICATE, ERR_HIGH_HASH, ERR_UNAUTHORIZED, ERR_NOT_SUBSCRIBED = 20, 21, 22, 23, 24, 25
ERROR_TEXT = {ERR_OTHER: "other", ERR_STALE: "job not found", ERR_DUPLICATE: "duplicate share",
              ERR_HIGH_HASH: "above the share target", ERR_UNAUTHORIZED: "unauthorized",
              ERR_NOT_SUBSCRIBED: "not subscribed"}


class StratumError(ValueError):
    """A message that breaks the format. `fatal`: the connection must be closed (an over-long
    line, or a line that is not a JSON object); otherwise the request is answered with `code`."""

    def __init__(self, message: str, code: int = ERR_OTHER, fatal: bool = False):
        super().__init__(message)
        self.code = code
        self.fatal = fatal


# ---------------------------------------------------------------------- hex fields
def strip0x(s) -> str:
    if not isinstance(s, str):
        raise StratumError("expected a hex string")
    return s[2:] if s[:2] in ("0x", "0X") else s


def parse_hex(s, digits: int, what: str) -> bytes:
    """`digits` hex digits, with or without 0x."""
    h = strip0x(s)
    if len(h) != digits:
        raise StratumError(f"{what}: expected {digits} hex digits, got {len(h)}")
    try:
        return bytes.fromhex(h)
    except ValueError:
        raise StratumError(f"{what}: not hexadecimal") from None


def parse_hash(s, what: str = "hash") -> bytes:
    return parse_hex(s, 64, what)


def parse_nonce(s) -> int:
    return int.from_bytes(parse_hex(s, 16, "nonce"), "big")


def parse_target(s) -> int:
    return int.from_bytes(parse_hex(s, 64, "target"), "big")


def target_hex(target: int) -> str:
    return "%064x" % target


def parse_extranonce(s) -> bytes:
    """0 to 12 hex digits, an even number of them."""
    if not isinstance(s, str):
        raise StratumError("extranonce: expected a hex string")
    if len(s) % 2 or len(s) > MAX_EXTRANONCE_DIGITS:
        raise StratumError(f"extranonce: {len(s)} hex digits (0 to {MAX_EXTRANONCE_DIGITS}, an even number)")
    try:
        return bytes.fromhex(s)
    except ValueError:
        raise StratumError("extranonce: not hexadecimal") from None


def share_target_for_bits(bits: int) -> int:
    """-stratumsharebits=n: 2^(256-n) - 1, the definition -minertargetbits uses."""
    return (1 << (256 - int(bits))) - 1


VARDIFF_MAX_STEP = 4   # bits per retarget, either way
VARDIFF_MAX_BITS = 255


def _floor_log2_ratio(a: int, b: int, cap: int) -> int:
    """min(cap, floor(log2(a / b))) for a >= b > 0: the largest k <= cap with a >= b << k."""
    k = 0
    while k < cap and a >= b << (k + 1):
        k += 1
    return k


def vardiff_next_bits(bits: int, shares: int, elapsed_ms: int, per_minute: int, lo_bits: int,
                      hi_bits: int = VARDIFF_MAX_BITS) -> int:
    """A connection's next share bits (the rule: module docstring). Integers only."""
    bits, shares, elapsed_ms, per_minute = int(bits), int(shares), int(elapsed_ms), int(per_minute)
    if shares < 0 or elapsed_ms < 0 or per_minute < 0:
        raise ValueError("vardiff: shares, elapsed_ms and per_minute must not be negative")
    e = per_minute * elapsed_ms
    s = shares * 60000
    if e > 0:
        if s >= 2 * e:
            bits += _floor_log2_ratio(s, e, VARDIFF_MAX_STEP)
        elif 2 * s <= e:
            bits -= VARDIFF_MAX_STEP if s == 0 else _floor_log2_ratio(e, s, VARDIFF_MAX_STEP)
    return max(int(lo_bits), min(int(hi_bits), bits))


# ---------------------------------------------------------------------- nonce ranges
def extranonce_range(extranonce: bytes) -> tuple[int, int]:
    """(nonce_base, free_bits): the extranonce bytes are the most significant bytes of the nonce."""
    free = 64 - 8 * len(extranonce)
    return int.from_bytes(extranonce, "big") << free if extranonce else 0, free


def nonce_in_extranonce(nonce: int, extranonce: bytes) -> bool:
    base, free = extranonce_range(extranonce)
    return 0 <= nonce < 1 << 64 and nonce >> free == base >> free


def rank_shift_for(free_bits: int, world_size: int) -> int:
    """s = free - ceil(log2(world_size)): 2^s nonces per rank, every rank inside the prefix. At most
    63, the largest shift a work packet carries: a single rank under an empty extranonce (64 free
    bits) searches the lower half of the nonce space."""
    s = min(63, int(free_bits) - max(0, int(world_size) - 1).bit_length())
    if s < 1:
        raise StratumError(f"{free_bits} free nonce bits cannot be split over {world_size} ranks")
    return s


# ---------------------------------------------------------------------- messages
@dataclass(frozen=True)
class Job:
    """One mining.notify."""
    job_id: str
    header_hash: bytes   # 32 bytes, ProgPoW order
    seed_hash: bytes     # 32 bytes
    target: int
    clean: bool
    height: int
    bits: int

    def params(self) -> list:
        return [self.job_id, self.header_hash.hex(), self.seed_hash.hex(), target_hex(self.target), bool(self.clean),
                int(self.height), "%08x" % self.bits]

    @classmethod
    def from_params(cls, p) -> "Job":
        if not isinstance(p, list) or len(p) < 7:
            raise StratumError("mining.notify: expected 7 params")
        job_id, hh, seed, target, clean, height, bits = p[:7]
        if not isinstance(job_id, str) or not job_id:
            raise StratumError("mining.notify: job_id must be a non-empty string")
        if not isinstance(clean, bool):
            raise StratumError("mining.notify: clean_jobs must be a boolean")
        if isinstance(height, bool) or not isinstance(height, int) or height < 0:
            raise StratumError("mining.notify: height must be a non-negative integer")
        return cls(job_id, parse_hash(hh, "header_hash"), parse_hash(seed, "seed_hash"), parse_target(target), clean,
                   height, int.from_bytes(parse_hex(bits, 8, "bits"), "big"))

    def work(self, job_id: int, nonce_base: int, flags: int):
        """The mining loop's work packet of this job: header = header hash, boundary = target."""
        from .search import Work

        return Work(self.header_hash, self.target.to_bytes(32, "big"), self.height, job_id, nonce_base, flags)


@dataclass(frozen=True)
class Submit:
    """One mining.submit."""
    user: str
    job_id: str
    nonce: int
    header_hash: bytes
    mix_hash: bytes

    def params(self) -> list:
        return [self.user, self.job_id, "0x%016x" % self.nonce, "0x" + self.header_hash.hex(),
                "0x" + self.mix_hash.hex()]

    @classmethod
    def from_params(cls, p) -> "Submit":
        if not isinstance(p, list) or len(p) < 5:
            raise StratumError("mining.submit: expected 5 params")
        user, job_id, nonce, hh, mix = p[:5]
        if not isinstance(user, str) or not isinstance(job_id, str):
            raise StratumError("mining.submit: user and job_id must be strings")
        return cls(user, job_id, parse_nonce(nonce), parse_hash(hh, "header_hash"), parse_hash(mix, "mix_hash"))


@dataclass(frozen=True)
class Message:
    """A decoded line. A request or notification has `method`; a response has none."""
    id: object = None
    method: str | None = None
    params: list | None = None
    result: object = None
    error: list | None = None

    @property
    def is_response(self) -> bool:
        return self.method is None

    @property
    def error_code(self) -> int | None:
        return int(self.error[0]) if self.error else None


def _line(obj: dict) -> bytes:
    return (json.dumps(obj, separators=(",", ":")) + "\n").encode()


def request(msg_id, method: str, params: list) -> bytes:
    return _line({"id": msg_id, "method": method, "params": params})


def notification(method: str, params: list) -> bytes:
    return _line({"id": None, "method": method, "params": params})


def response(msg_id, result) -> bytes:
    return _line({"id": msg_id, "result": result, "error": None})


def error_response(msg_id, code: int, message: str | None = None) -> bytes:
    return _line({"id": msg_id, "result": None, "error": [int(code), message or ERROR_TEXT.get(code, "error"), None]})


def subscribe(msg_id, agent: str) -> bytes:
    return request(msg_id, "mining.subscribe", [agent])


def authorize(msg_id, user: str, password: str) -> bytes:
    return request(msg_id, "mining.authorize", [user, password])


def submit(msg_id, s: Submit) -> bytes:
    return request(msg_id, "mining.submit", s.params())


def notify(job: Job) -> bytes:
    return notification("mining.notify", job.params())


def set_target(target: int) -> bytes:
    return notification("mining.set_target", [target_hex(target)])


def subscribe_result(session, extranonce: bytes) -> list:
    return [session, extranonce.hex()]


def parse_subscribe_result(result) -> tuple[object, bytes]:
    if not isinstance(result, list) or len(result) < 2:
        raise StratumError("mining.subscribe: expected [session, extranonce]")
    return result[0], parse_extranonce(result[1])


def parse_set_target(params) -> int:
    if not isinstance(params, list) or not params:
        raise StratumError("mining.set_target: expected [target]")
    return parse_target(params[0])


def decode(line: bytes | str) -> Message:
    """One line (without or with its newline) -> Message. StratumError(fatal=True) for a line
    longer than 16 KiB or one that is not a JSON object."""
    raw = line.encode() if isinstance(line, str) else bytes(line)
    if len(raw) > MAX_LINE:
        raise StratumError("line longer than 16 KiB", fatal=True)
    try:
        obj = json.loads(raw.decode("utf-8"))
    except (UnicodeDecodeError, ValueError):
        raise StratumError("not JSON", fatal=True) from None
    if not isinstance(obj, dict):
        raise StratumError("not a JSON object", fatal=True)
    method = obj.get("method")
    if method is not None:
        if not isinstance(method, str):
            raise StratumError("method must be a string")
        params = obj.get("params")
        if params is None:
            params = []
        if not isinstance(params, list):
            raise StratumError("params must be an array")
        return Message(obj.get("id"), method, params)
    err = obj.get("error")
    if err is not None and not (isinstance(err, list) and err and isinstance(err[0], int)):
        raise StratumError("error must be null or [code, message, null]")
    return Message(obj.get("id"), None, None, obj.get("result"), err)


class LineBuffer:
    """Bytes from a socket -> whole lines. StratumError(fatal=True) once an unterminated line
    exceeds 16 KiB."""

    def __init__(self):
        self.buf = bytearray()

    def feed(self, data: bytes) -> list[bytes]:
        self.buf += data
        out = []
        while True:
            i = self.buf.find(b"\n")
            if i < 0:
                break
            if i > MAX_LINE:
                raise StratumError("line longer than 16 KiB", fatal=True)
            line = bytes(self.buf[:i])
            del self.buf[:i + 1]
            if line.strip():
                out.append(line)
        if len(self.buf) > MAX_LINE:
            raise StratumError("line longer than 16 KiB", fatal=True)
        return out
