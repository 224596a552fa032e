"""The discrete-event draws of csrc/device_rng.hpp (NormalStream::exponential_pair, event_pair, while_events, poisson,
binomial) and the simulators built on them, restated in Python over the oracle's Philox blocks (O.stream_block, O.u52) with
math.log / math.lgamma / math.exp: the same algorithms, the same constants, the same block accounting -- every draw consumes
whole blocks of one (seed, particle, purpose, iteration) stream, in order."""
import math


class Stream:
    """Block k of the stream gives (u0, u1) = (u52(w0, w1), u52(w2, w3)), as NormalStream::uniform_pair does."""

    def __init__(self, O, seed, pid, it, purpose=None, k=0):
        self.O, self.seed, self.pid, self.it, self.k = O, int(seed), int(pid), int(it), int(k)
        self.purpose = O.PURPOSE_SIM if purpose is None else purpose

    def uniform_pair(self):
        w = self.O.stream_block(self.seed, self.pid, self.purpose, self.it, self.k)
        self.k += 1
        return self.O.u52(w[0], w[1]), self.O.u52(w[2], w[3])

    def normal_pair(self):
        z = self.O.normal_pair(self.seed, self.pid, self.purpose, self.it, self.k)
        self.k += 1
        return float(z[0]), float(z[1])

    def exponential_pair(self):
        u0, u1 = self.uniform_pair()
        return -math.log(u0), -math.log(u1)

    def event_pair(self):
        u0, u1 = self.uniform_pair()
        return -math.log(u0), u1

    def while_events(self, max_events, f):
        count = 0
        while count < max_events:
            e, u = self.event_pair()
            count += 1
            if not f(e, u):
                break
        return count

    def poisson(self, lam):
        if not lam > 0.0:
            return 0
        if lam < 10.0:
            u, _ = self.uniform_pair()
            p = math.exp(-lam)
            c, k = p, 0
            while u >= c and k < 1000:
                k += 1
                p *= lam / k
                c += p
            return k
        b = 0.931 + 2.53 * math.sqrt(lam)
        a = -0.059 + 0.02483 * b
        inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        log_lam = math.log(lam)
        for _ in range(64):
            u, v = self.uniform_pair()
            U = u - 0.5
            us = 0.5 - abs(U)
            k = math.floor((2.0 * a / us + b) * U + lam + 0.43)
            if us >= 0.07 and v <= vr:
                return k
            if k < 0 or (us < 0.013 and v > us):
                continue
            if math.log(v) + math.log(inv_alpha) - math.log(a / (us * us) + b) <= -lam + k * log_lam - math.lgamma(k + 1.0):
                return k
        return math.floor(lam)

    def binomial(self, n, p):
        n = int(n)
        if n <= 0 or not p > 0.0:
            return 0
        if p >= 1.0:
            return n
        if p > 0.5:
            return n - self._binomial_lower(n, 1.0 - p)
        return self._binomial_lower(n, p)

    def _binomial_lower(self, n, p):
        q = 1.0 - p
        r = p / q
        if n * p < 10.0:
            u, _ = self.uniform_pair()
            pk = math.exp(n * math.log(q))
            c, k = pk, 0
            while u >= c and k < n and k < 1000:
                k += 1
                pk *= r * (n - k + 1) / k
                c += pk
            return k
        spq = math.sqrt(n * p * q)
        b = 1.15 + 2.53 * spq
        a = -0.0873 + 0.0248 * b + 0.01 * p
        c = n * p + 0.5
        vr = 0.92 - 4.2 / b
        alpha = (2.83 + 5.1 / b) * spq
        m = math.floor((n + 1.0) * p)
        log_r = math.log(r)
        h = math.lgamma(m + 1.0) + math.lgamma(n - m + 1.0)
        for _ in range(64):
            u, v = self.uniform_pair()
            U = u - 0.5
            us = 0.5 - abs(U)
            k = math.floor((2.0 * a / us + b) * U + c)
            if us >= 0.07 and v <= vr:
                return k
            if k < 0 or k > n:
                continue
            if math.log(v * alpha / (a / (us * us) + b)) <= h - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0) + (k - m) * log_r:
                return k
        return m


def sir_statistics(rng, beta, gamma, S0, I0, R0, t_max):
    """device_sources/sir.hip (docs/src/example.md:75-173 of the reference): final R, peak I and the time of the peak; event j
    is block j of the stream."""
    N = float(S0 + I0 + R0)
    st = dict(S=S0, I=I0, R=R0, t=0.0, peak=I0, t_peak=0.0)

    def event(e, u):
        infection_rate = beta * st["S"] * st["I"] / N
        recovery_rate = gamma * st["I"]
        total_rate = infection_rate + recovery_rate
        if not total_rate > 0.0:
            return False
        st["t"] += e / total_rate
        if u < infection_rate / total_rate:
            st["S"] -= 1
            st["I"] += 1
        else:
            st["I"] -= 1
            st["R"] += 1
        if st["I"] > st["peak"]:
            st["peak"], st["t_peak"] = st["I"], st["t"]
        return st["t"] < t_max and st["I"] > 0

    if st["t"] < t_max and st["I"] > 0:
        rng.while_events(2 * S0 + I0, event)
    return float(st["R"]), float(st["peak"]), st["t_peak"]


def sir_distances(O, seed, pid, it, theta, params, n_stats):
    """rho of StochasticSIR for particle `pid` at iteration `it`; params = [S0, I0, R0, t_max, obs x 3]."""
    S0, I0, R0 = int(params[0]), int(params[1]), int(params[2])
    stats = sir_statistics(Stream(O, seed, pid, it), float(theta[0]), float(theta[1]), S0, I0, R0, float(params[3]))
    d = [(a - b) ** 2 for a, b in zip(stats, params[4:7])]
    return tuple(d) if n_stats == 3 else (d[0] + d[1] + d[2],)
