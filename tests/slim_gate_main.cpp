// Stand-alone driver of csrc/slim_gate.h for tests/test_slim_gate.py: built with g++ and the host sanitizers, run as a child process,
// one role per invocation (argv[1]).  No GPU, no HIP runtime; the knobs (lock directory, NO_OWNER_GATE, GATE_WAIT_S) come from the
// environment the test sets, through read_slim_knobs.  A role that checks something itself prints "ok" last and exits 0; a failed
// CHECK prints the expression and exits 1.  The roles that another process is played against talk over stdin / stdout, a line each.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/slim_gate.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>

using namespace mi355rec;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("CHECK failed, line %d: %s\n", __LINE__, #cond);       \
            fflush(stdout);                                                \
            _exit(1);                                                      \
        }                                                                  \
    } while (0)

static const std::string BUS = "0000:c1:00.0";        // (':' and '.' become '_' in the file's name)
static std::string g_self;

static void say(const std::string &line) {
    printf("%s\n", line.c_str());
    fflush(stdout);
}
static std::string hear() {
    std::string line;
    std::getline(std::cin, line);
    return line;
}
// what a fresh process answers to acquire() right now: "granted" / "denied"
static std::string second_process_says() {
    FILE *p = popen((g_self + " probe").c_str(), "r");
    CHECK(p != nullptr);
    char buf[64] = "";
    CHECK(fgets(buf, sizeof(buf), p) != nullptr);
    CHECK(pclose(p) == 0);
    buf[strcspn(buf, "\n")] = 0;
    return buf;
}
static bool serial_is_free(OwnerGate &g) {
    bool free = false;
    std::thread([&] {                                  // (try_lock from the thread that holds a std::mutex is undefined)
        free = g.serial.try_lock();
        if (free) g.serial.unlock();
    }).join();
    return free;
}

static int probe(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    const bool got = g.acquire(k, BUS);
    say(got ? "granted" : "denied");
    if (got) g.release();
    return 0;
}

// acquire, say so, then do what stdin says: "release" (and go on listening) or "exit" (with the gate held: the kernel drops the lock)
static int hold(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    say(g.acquire(k, BUS) ? "held" : "denied");
    for (;;) {
        const std::string line = hear();
        if (line == "release") {
            g.release();
            say("released");
        } else {
            _exit(0);
        }
    }
}

static int nesting(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    CHECK(g.acquire(k, BUS));
    const int fd = g.fd;
    CHECK(fd >= 0 && g.holders == 1);
    CHECK(g.acquire(k, BUS));
    CHECK(g.fd == fd && g.holders == 2);               // one file lock for both
    CHECK(second_process_says() == "denied");
    g.release();
    CHECK(g.fd == fd && g.holders == 1);
    CHECK(second_process_says() == "denied");
    g.release();
    CHECK(g.fd == -1 && g.holders == 0);               // dropped with the last holder
    CHECK(second_process_says() == "granted");
    g.release();                                       // one release too many changes nothing
    CHECK(g.fd == -1 && g.holders == 0);
    CHECK(g.acquire_blocking(k, BUS));                 // the blocking flavour takes the same lock ...
    CHECK(g.fd >= 0 && g.holders == 1 && !serial_is_free(g));
    CHECK(second_process_says() == "denied");
    CHECK(g.acquire(k, BUS) && g.holders == 2);        // ... and a dense launch of the process nests inside it
    g.release();
    g.release_blocking();
    CHECK(g.fd == -1 && g.holders == 0 && serial_is_free(g));
    CHECK(second_process_says() == "granted");
    say("ok");
    return 0;
}

// MI355REC_SLIM_NO_OWNER_GATE: always granted, no file (the test looks into the directory)
static int no_gate(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    CHECK(k.no_owner_gate);
    CHECK(g.acquire(k, BUS) && g.fd == -1 && g.holders == 1);
    CHECK(second_process_says() == "granted");
    g.release();
    CHECK(g.acquire_blocking(k, BUS) && g.fd == -1 && g.holders == 1);
    g.release_blocking();
    CHECK(g.holders == 0 && serial_is_free(g));
    OwnerLease lease;
    lease.take(true, 64, 256, k, BUS);
    CHECK(lease.slots == 64 && lease.gated);
    lease.give_back();
    say("ok");
    return 0;
}

// the lock file cannot be opened (the test makes its path a symbolic link, or the directory one that does not exist)
static int no_lock_file(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    CHECK(OwnerGate::open_lock_file(k, BUS) < 0);
    CHECK(!g.acquire(k, BUS) && g.fd == -1 && g.holders == 0);          // no owners
    OwnerLease lease;
    lease.take(true, 256, 256, k, BUS);
    CHECK(lease.slots == 0 && !lease.gated);                            // queue-only launch
    CHECK(g.acquire_blocking(k, BUS));                                  // serialised inside the process only
    CHECK(g.fd == -1 && g.holders == 1 && !serial_is_free(g));
    g.release_blocking();
    CHECK(g.holders == 0 && serial_is_free(g));
    say("ok");
    return 0;
}

// against a holder in another process: the timeout is reported and leaves `serial` unlocked; once stdin says the holder is gone, the
// next call gets the lock
static int blocking(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    try {
        g.acquire_blocking(k, BUS);
        say("held at once");
        return 1;
    } catch (const GateTimeout &t) {
        char line[64];
        snprintf(line, sizeof(line), "timeout %.3f", t.wait_s);
        say(line);
    }
    CHECK(serial_is_free(g) && g.fd == -1 && g.holders == 0);
    say("serial free");
    hear();
    CHECK(g.acquire_blocking(k, BUS) && g.fd >= 0 && g.holders == 1);
    say("held");
    g.release_blocking();
    CHECK(g.fd == -1 && serial_is_free(g));
    say("ok");
    return 0;
}

// two threads: their critical sections never overlap
static int threads(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    std::atomic<int> inside{0}, overlaps{0}, rounds{0};
    int plain = 0;                                     // (unsynchronised but for the gate: what a race detector watches)
    const auto work = [&] {
        for (int r = 0; r < 20; ++r) {
            if (!g.acquire_blocking(k, BUS)) overlaps += 1000;
            if (inside.fetch_add(1) != 0) ++overlaps;
            ++plain;
            usleep(200);
            inside.fetch_sub(1);
            ++rounds;
            g.release_blocking();
        }
    };
    std::thread a(work), b(work);
    a.join();
    b.join();
    CHECK(overlaps == 0 && rounds == 40 && plain == 40);
    CHECK(g.fd == -1 && g.holders == 0 && serial_is_free(g));
    say("ok");
    return 0;
}

// the slot pool of a device with 256 compute units
static int lease(const SlimKnobs &k) {
    OwnerGate &g = owner_gate();
    const int cus = 256;
    {
        OwnerLease none;
        none.take(false, 256, cus, k, BUS);            // not wanted: nothing taken, the gate untouched
        CHECK(none.slots == 0 && !none.gated && g.holders == 0 && owner_slots().load() == -1);
    }
    {
        OwnerLease a, b;
        a.take(true, 256, cus, k, BUS);
        b.take(true, 64, cus, k, BUS);
        CHECK(a.slots == 256 && b.slots == 0 && b.gated);              // the second launch: queue-only
        CHECK(g.holders == 2 && owner_slots().load() == 0);
        a.give_back();
        CHECK(owner_slots().load() == 256 && g.holders == 1 && g.fd >= 0);
        a.give_back();                                                  // twice: harmless
        CHECK(owner_slots().load() == 256 && g.holders == 1);
        b.give_back();
        CHECK(g.holders == 0 && g.fd == -1);
    }
    {
        OwnerLease a, b, c;
        a.take(true, 128, cus, k, BUS);
        b.take(true, 128, cus, k, BUS);
        c.take(true, 64, cus, k, BUS);
        CHECK(a.slots == 128 && b.slots == 128 && c.slots == 0);
    }                                                                   // (the destructors give everything back)
    CHECK(owner_slots().load() == 256 && g.holders == 0 && g.fd == -1);
    {
        OwnerLease a, b, c;
        a.take(true, 225, cus, k, BUS);
        b.take(true, 64, cus, k, BUS);
        CHECK(a.slots == 225 && b.slots == 0 && owner_slots().load() == 31);      // 31 left: nothing is handed out
        a.give_back();
        c.take(true, 300, cus, k, BUS);
        CHECK(c.slots == 256);                                          // never more than there are
    }
    CHECK(owner_slots().load() == 256 && g.holders == 0 && g.fd == -1);
    CHECK(second_process_says() == "granted");
    say("ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    g_self = argv[0];
    const SlimKnobs k = read_slim_knobs();
    const std::string role = argv[1];
    if (role == "probe") return probe(k);
    if (role == "hold") return hold(k);
    if (role == "nesting") return nesting(k);
    if (role == "no_gate") return no_gate(k);
    if (role == "no_lock_file") return no_lock_file(k);
    if (role == "blocking") return blocking(k);
    if (role == "threads") return threads(k);
    if (role == "lease") return lease(k);
    return 2;
}
