// ttga-ga: the reference's ga.cpp driver (ga.cpp:370-613) as a native host
// program over the C-ABI of include/ttga.h. One island per GPU of this node;
// the MPI island model becomes RCCL over xGMI (one host thread and one
// communicator rank per GPU, ncclCommInitAll), the OpenMP threads of a rank
// become C children bred per batched generation. With --islands K != --gpus,
// island g runs on GPU g % gpus and migrants move by device copies (the same
// ring, no communicator): K islands can share one GPU. --rccl takes the RCCL
// path for one island on one GPU too (a one-rank communicator: the ring's
// send/recv pairs go to the rank itself), so the communicator's calls run on a
// one-GPU box.
//
//   ttga-ga -i instance.tim [-s seed] [-p type] [-c children]
//           [-p1 x -p2 y -p3 z] [--gpus G] [--islands K] [--pop N] [--generations n] [--rccl] [--stagger]
//           [--report] [--unique] [--init random|greedy] [--kempe P] [--kempe-max-chain N]
//           [--slot-swap N] [--lahc N] [--lahc-history L] [--lahc-swap P]
//           [--lahc-kempe P] [--lahc-kempe-max-chain N] [--lahc-kempe-rooms direct|augment]
//           [--lahc-walkers K] [--move1-descent N]
//           [--crossover uniform|guided] [--crossover-repair]
//
// --crossover guided: every sub-batch is bred by tt_ga_breed_guided
// (include/ttga_cx.h) in place of tt_ga_breed, in tt_greedy_order's event order;
// with --crossover-repair an event that clashes in both parents' slots goes to a
// slot of least cost. Each island then prints one {"crossover": {"children",
// "clean", "crossed", "meanCost", "repaired"}} line directly after its solution
// line, before a kempe line (ttga.islands prints the same). The default is
// uniform: no new call.
//
// --lahc N: tt_lahc (include/ttga_lahc.h) with N steps, history L (--lahc-history,
// default 500) and swap probability P (--lahc-swap, default 0.5) runs directly
// behind every tt_local_search_eval, and behind tt_slot_swap when that is on, on
// the same stream: on every sub-batch of children with the children's own
// streams, on the members with the initial streams before the initial sort. Rows
// that are feasible walk and come back as the best row of the walk, their scv
// and penalty lowered in place. Each island then prints one {"lahc": {"accepted",
// "gain", "improved", "rows", "searched"}} line after the slotSwap line
// (ttga.islands prints the same). The default is 0: no call.
//
// --lahc-kempe P (needs --lahc, and --lahc-swap + P <= 1): the walk is
// tt_lahc_kempe (include/ttga_lahc_kempe.h) in place of tt_lahc, with a share P
// of Kempe-chain candidates of at most --lahc-kempe-max-chain N events (0, the
// default: no cap). Each island then prints one {"lahcKempe": {"accepted",
// "capped", "meanChain", "noRoom", "tried"}} line after its lahc line
// (ttga.islands prints the same). The default is 0: tt_lahc as before.
//
// --lahc-kempe-rooms augment (needs --lahc-kempe P > 0): the walk is
// tt_lahc_kempe_aug (include/ttga_lahc_kempe_aug.h) with room_rule 1 in place of
// tt_lahc_kempe: a chain event with no free possible room moves the target
// slot's holders along an augmenting path. The lahcKempe line then also carries
// "rescued" and "displaced". The default is direct: no new call.
//
// --lahc-walkers K (1 .. 1024, needs --lahc; the default is 1: no new call): with K > 1 the
// walk is tt_lahc_multi (include/ttga_lahc_multi.h) with the walk's other flags: K walks
// from every row, each on its own stretch of the row's stream, the best one kept. The lahc
// and lahcKempe lines then describe the winners' walks, and each island prints one
// {"lahcWalkers": {"gain", "gainFirst", "rows", "walkers", "winnerLater"}} line after them
// (ttga.islands prints the same): the rows that walked, the winners' gain, walker 0's gain
// on the same rows (the single walk's) and the rows another walker won.
//
// --move1-descent N: tt_move1_descent (include/ttga/move1.h) with max_passes N runs
// directly behind every tt_local_search_eval, and behind tt_slot_swap and the walk
// where those are on, on the same stream: on every sub-batch of children, on the
// members before the initial sort. On every feasible row the feasible single-event
// move that lowers scv most is applied, at most N times, and the rows' scv and
// penalty are lowered in place. Each island then prints one {"move1Descent":
// {"gain", "improved", "meanPasses", "rows"}} line after the lahc, lahcKempe and
// lahcWalkers lines and before any report line (ttga.islands prints the same). The
// default is 0: no call.
//
// --slot-swap N: tt_slot_swap (include/ttga_slotswap.h) with max_passes N runs
// directly behind every tt_local_search_eval, on the same stream, and lowers
// the searched rows' scv and penalty in place: on every sub-batch of children
// before its replacement, on the members before the initial sort. Each island
// then prints one {"slotSwap": {"gain", "improved", "meanPasses", "rows"}} line
// after the solution, kempe and unique lines (ttga.islands prints the same).
// The default is 0: no call.
//
// --kempe P: every child gets tt_kempe_move (include/ttga_kempe.h) with
// probability P directly after tt_ga_breed and before its search, on its own
// stream; --kempe-max-chain N refuses chains of more than N events (0, the
// default: no cap). Each island then prints one
// {"kempe": {"children", "meanChain", "moved", "rejected"}} line after its
// solution line (ttga.islands prints the same). The default is 0: no call.
//
// --init greedy: the initial population is built by tt_greedy_init
// (include/ttga_greedy.h) instead of RandomInitialSolution (ga.cpp:431); the
// local search and the sort after it are unchanged. The default is random.
//
// --unique: duplicate-free replacement (include/ttga_unique.h): a child whose
// genome is already in the population, or in an earlier child of its sub-batch,
// is dropped on the device. After the solution lines and before any report
// line, one `unique` line per island: children bred, children dropped, distinct
// genomes left (the same line as python -m ttga.islands --unique prints).
// Migration is unchanged: a migrant may duplicate a member of its destination.
//
// --report: after the solution lines, one `report` line per island: the best
// member's six constraint parts, their sums over the population and its slot
// diversity (include/ttga_report.h; the same line as ttga/report.py prints).
//
// --stagger / --stagger-parts P: the children of a generation are 2 / P
// sub-batches on as many streams, sub-batch h bred from the population after
// the replacement of sub-batch h - P (ttga/ga.py Island, schedule "staggered";
// same results as the Python driver with the same option).
//
// Reference correspondence:
//  * CLI: `-key value` pairs and messages of Control::Control (Control.cpp:3-137);
//    -o -n -t -m -l are parsed and echoed, then ignored, as in ga.cpp (output
//    always goes to stdout, ga.cpp:60).
//  * -p -> maxSteps 200 / 1000 / 2000 (ga.cpp:389-397).
//  * island k runs with seed abs(seed + k*(seed/10)) (ga.cpp:412); all islands
//    start from island 0's initial population (ga.cpp:429-444,463-464).
//  * generation loop, migration before generations g with (g+1) % 100 == 50,
//    best -> right neighbour's pop[N-1], 2nd best -> left neighbour's pop[N-2]
//    (ga.cpp:479-540); MIN all-reduce of the best value (ga.cpp:234-257);
//    JSON lines of endTry / setCurrentCost / runEntry (ga.cpp:169-228,602-609)
//    in jsoncpp's compact format (sorted keys, doubles as %.17g); logEntry
//    threadID = the child slot whose replacement made the new best (ga.cpp:584);
//    logEntry/solution times from beginTry (ga.cpp:476), the last totalTime
//    from process start (ga.cpp:381).
//  * same stream layout as ttga/ga.py (Island): member i of the initial
//    population draws from Random(|s|+1+i), child slot c from Random(|s|+1+N+c).
#include <rccl/rccl.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ttga_report.h"
#include "../../include/ttga_greedy.h"
#include "../../include/ttga_kempe.h"
#include "../../include/ttga_slotswap.h"
#include "../../include/ttga_lahc.h"
#include "../../include/ttga_cx.h"
#include "../../include/ttga_unique.h"
#include "../../include/ttga/move1.h"

namespace {

[[noreturn]] void die(const std::string& msg) {
    std::cerr << "ttga-ga: " << msg << std::endl;
    std::exit(1);
}

void check_tt(int rc, const char* what) {
    if (rc != TT_OK) die(std::string(what) + ": " + tt_last_error());
}

void check_hip(hipError_t e, const char* what) {
    if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e));
}

void check_nccl(ncclResult_t r, const char* what) {
    if (r != ncclSuccess) die(std::string(what) + ": " + ncclGetErrorString(r));
}

// ---------------------------------------------------------------- Control
const char* kUsage = " -i InputFile [-o OutputFile] [-n NumberOfTries] [-s RandomSeed] [-t TimeLimit] [-p ProblemType]";

// The optional stages' settings (ttga/stages.py lists the same flags)
struct Stages {
    bool unique = false;                          // --unique: duplicate-free replacement, a unique line per island
    bool greedy = false;                          // --init greedy: tt_greedy_init builds the initial population
    double kempe = 0.0;                           // --kempe: tt_kempe_move's probability (0: never called)
    int kempe_max_chain = 0;                      // --kempe-max-chain (0: no cap)
    int slot_swap = 0;                            // --slot-swap: tt_slot_swap's max_passes (0: never called)
    int lahc = 0;                                 // --lahc: tt_lahc's steps (0: never called)
    int lahc_history = 500;                       // --lahc-history
    double lahc_swap = 0.5;                       // --lahc-swap
    double lahc_kempe = 0.0;                      // --lahc-kempe: tt_lahc_kempe's share of chains (0: tt_lahc)
    int lahc_kempe_max_chain = 0;                 // --lahc-kempe-max-chain (0: no cap)
    bool lahc_kempe_augment = false;              // --lahc-kempe-rooms augment: tt_lahc_kempe_aug, room_rule 1
    int lahc_walkers = 1;                         // --lahc-walkers: tt_lahc_multi's walkers (1: the calls above)
    bool guided = false;                          // --crossover guided: tt_ga_breed_guided breeds
    bool cx_repair = false;                       // --crossover-repair
    int move1_descent = 0;                        // --move1-descent: tt_move1_descent's max_passes (0: never called)
};

struct Control {
    int threads = 1, tries = 10, problem_type = 1, max_steps = 100;
    double time_limit = 90, ls_limit = 99999, p1 = 1.0, p2 = 1.0, p3 = 0.0;
    long seed = 0;
    std::string input, output;
    int gpus = 1, islands = 0, pop = 10, generations = -1;
    bool rccl = false;
    int stagger = 0;                              // sub-batches of the staggered schedule (0: batch)
    bool report = false;                          // a population report line per island
    Stages stage;
};

// The extensions' flags are stripped from the arguments, with their values, before
// Control.cpp's pair count; a missing or bad value prints the flag's message and exits with 1.
using Args = std::vector<std::string>;

[[noreturn]] void bad_flag(const char* msg) {
    std::cerr << "Error: " << msg << std::endl;
    std::exit(1);
}

// a bare flag: true when it was there
bool take_flag(Args& args, const char* flag) {
    auto it = std::find(args.begin(), args.end(), flag);
    if (it == args.end()) return false;
    args.erase(it);
    return true;
}

// The word behind the flag at `it` as a number; a NaN, which fails every range check, where
// there is none, where it is empty (unless empty_is_0: strtod's reading) or is not a number
// to its last character
double number_behind(const Args& args, Args::const_iterator it, bool empty_is_0) {
    if (it + 1 == args.end() || ((it + 1)->empty() && !empty_is_0)) return NAN;
    char* end = nullptr;
    const double v = std::strtod((it + 1)->c_str(), &end);
    return *end ? NAN : v;
}

// `flag N` with an integer N >= low
void take_int(Args& args, const char* flag, int low, const char* msg, int& dst, bool empty_is_0 = false) {
    auto it = std::find(args.begin(), args.end(), flag);
    if (it == args.end()) return;
    const double v = number_behind(args, it, empty_is_0);
    if (!(v >= low && v == std::floor(v) && v <= INT_MAX)) bad_flag(msg);
    dst = (int)v;
    args.erase(it, it + 2);
}

// `flag P` with a probability P
void take_prob(Args& args, const char* flag, const char* msg, double& dst, bool empty_is_0 = false) {
    auto it = std::find(args.begin(), args.end(), flag);
    if (it == args.end()) return;
    const double v = number_behind(args, it, empty_is_0);
    if (!(v >= 0.0 && v <= 1.0)) bad_flag(msg);
    dst = v;
    args.erase(it, it + 2);
}

// `flag first|second`: dst is whether it was the second word
void take_choice(Args& args, const char* flag, const char* first, const char* second, const char* msg, bool& dst) {
    auto it = std::find(args.begin(), args.end(), flag);
    if (it == args.end()) return;
    if (it + 1 == args.end() || (*(it + 1) != first && *(it + 1) != second)) bad_flag(msg);
    dst = *(it + 1) == second;
    args.erase(it, it + 2);
}

// Control::Control (Control.cpp:3-137) plus the --gpus/--pop/--generations extensions.
Control parse_control(int argc, char** argv) {
    Args args(argv + 1, argv + argc);
    Control c;
    Stages& s = c.stage;
    c.rccl = take_flag(args, "--rccl");
    if (take_flag(args, "--stagger")) c.stagger = 2;
    c.report = take_flag(args, "--report");
    s.unique = take_flag(args, "--unique");
    take_choice(args, "--init", "random", "greedy", "--init must be random or greedy", s.greedy);
    // these two alone read an empty word as 0
    const char* kempe_msg = "--kempe must be a probability in [0, 1], --kempe-max-chain an integer >= 0";
    take_prob(args, "--kempe", kempe_msg, s.kempe, true);
    take_int(args, "--kempe-max-chain", 0, kempe_msg, s.kempe_max_chain, true);
    take_int(args, "--slot-swap", 0, "--slot-swap must be a non-negative integer", s.slot_swap);
    take_int(args, "--lahc", 0, "--lahc must be a non-negative integer", s.lahc);
    take_int(args, "--lahc-history", 1, "--lahc-history must be a positive integer", s.lahc_history);
    take_prob(args, "--lahc-swap", "--lahc-swap must be a probability in [0, 1]", s.lahc_swap);
    take_prob(args, "--lahc-kempe", "--lahc-kempe must be a probability in [0, 1]", s.lahc_kempe);
    take_int(args, "--lahc-kempe-max-chain", 0, "--lahc-kempe-max-chain must be a non-negative integer",
             s.lahc_kempe_max_chain);
    take_choice(args, "--lahc-kempe-rooms", "direct", "augment", "--lahc-kempe-rooms must be direct or augment",
                s.lahc_kempe_augment);
    take_int(args, "--lahc-walkers", 1, "--lahc-walkers must be an integer from 1 to 1024", s.lahc_walkers);
    if (s.lahc_walkers > 1024) bad_flag("--lahc-walkers must be an integer from 1 to 1024");
    s.cx_repair = take_flag(args, "--crossover-repair");
    take_choice(args, "--crossover", "uniform", "guided", "--crossover must be uniform or guided", s.guided);
    take_int(args, "--move1-descent", 0, "--move1-descent must be a non-negative integer", s.move1_descent);
    if (s.cx_repair && !s.guided) bad_flag("--crossover-repair needs --crossover guided");
    if (s.lahc_kempe > 0 && s.lahc <= 0) bad_flag("--lahc-kempe needs --lahc");
    if (s.lahc_kempe > 0 && !(s.lahc_swap <= 1.0 - s.lahc_kempe))         // tt_lahc_kempe's own test
        bad_flag("--lahc-swap and --lahc-kempe must not add up to more than 1");
    if (s.lahc_kempe_augment && !(s.lahc_kempe > 0)) bad_flag("--lahc-kempe-rooms augment needs --lahc-kempe");
    if (s.lahc_walkers > 1 && s.lahc <= 0) bad_flag("--lahc-walkers needs --lahc");
    for (const char* k : {"--gpus", "--islands", "--pop", "--generations", "--children", "--stagger-parts"}) {
        auto it = std::find(args.begin(), args.end(), k);
        if (it != args.end()) {
            if (it + 1 == args.end()) die(std::string("missing value for ") + k);
            const int v = std::atoi((it + 1)->c_str());
            if (!std::strcmp(k, "--gpus")) c.gpus = v;
            else if (!std::strcmp(k, "--islands")) c.islands = v;
            else if (!std::strcmp(k, "--pop")) c.pop = v;
            else if (!std::strcmp(k, "--generations")) c.generations = v;
            else if (!std::strcmp(k, "--stagger-parts")) c.stagger = v;
            else c.threads = v;
            args.erase(it, it + 2);
        }
    }
    if (args.empty() || args.size() % 2 != 0) {
        std::cerr << "Parse error: Number of command line parameters incorrect\n";
        std::cerr << "Usage:" << std::endl << argv[0] << kUsage << std::endl;
        std::exit(1);
    }
    std::map<std::string, std::string> kv;
    for (size_t i = 0; i + 1 < args.size(); i += 2) kv[args[i]] = args[i + 1];
    auto has = [&](const char* k) { return kv.count(k) > 0; };
    if (has("-c")) {
        c.threads = std::atoi(kv["-c"].c_str());
        std::cout << "Max number of threads " << c.threads << std::endl;
    } else {
        std::cerr << "Warning: Number of threads is set to default (1)" << std::endl;
    }
    if (!has("-i")) {
        std::cerr << "Error: No input file given, exiting" << std::endl;
        std::cerr << "Usage:" << std::endl << argv[0] << kUsage << std::endl;
        std::exit(1);
    }
    c.input = kv["-i"];
    if (has("-o")) c.output = kv["-o"];
    else std::cerr << "Warning: No output file given, writing to stdout" << std::endl;
    if (has("-n")) {
        c.tries = std::atoi(kv["-n"].c_str());
        std::cout << "Max number of tries " << c.tries << std::endl;
    } else {
        std::cerr << "Warning: Number of tries is set to default (10)" << std::endl;
    }
    if (has("-t")) {
        c.time_limit = std::atof(kv["-t"].c_str());
        std::cout << "Time limit " << c.time_limit << std::endl;
    } else {
        std::cerr << "Warning: Time limit is set to default (90 sec)" << std::endl;
    }
    if (has("-p")) {
        c.problem_type = std::atoi(kv["-p"].c_str());
        std::cout << "Problem instance type " << c.problem_type << std::endl;
    }
    if (has("-m")) {
        c.max_steps = std::atoi(kv["-m"].c_str());
        std::cout << "Max number of steps in the local search " << c.max_steps << std::endl;
    }
    if (has("-l")) {
        c.ls_limit = std::atof(kv["-l"].c_str());
        std::cout << "Local search time limit " << c.ls_limit << std::endl;
    } else {
        std::cerr << "Warning: The local search time limit is set to default (99999 sec)" << std::endl;
    }
    struct P { const char* key; double* dst; const char* dflt; int n; };
    for (P p : {P{"-p1", &c.p1, "1.0", 1}, P{"-p2", &c.p2, "1.0", 2}, P{"-p3", &c.p3, "0.0", 3}}) {
        if (has(p.key)) {
            *p.dst = std::atof(kv[p.key].c_str());
            std::cout << "LS move " << p.n << " probability " << *p.dst << std::endl;
        } else {
            std::cerr << "Warning: The local search move " << p.n << " probability is set to default " << p.dflt
                      << std::endl;
        }
    }
    if (has("-s")) {
        c.seed = std::atol(kv["-s"].c_str());
    } else {
        c.seed = (long)std::time(nullptr);
        std::cerr << "Warning: " << c.seed << " used as default random seed" << std::endl;
    }
    return c;
}

// ga.cpp:389-397
int max_steps_for(int problem_type) { return problem_type == 1 ? 200 : problem_type == 2 ? 1000 : 2000; }

// ga.cpp:412 (C int division)
long island_seed(long seed, int k) { return std::labs(seed + k * (seed / 10)); }

// ---------------------------------------------------------------- .tim
struct Instance {
    int E = 0, R = 0, F = 0, S = 0;
    std::vector<int32_t> room_size, student_events, room_features, event_features;
};

// Problem::Problem(istream&) token order (Problem.cpp:7-74).
Instance read_tim(const std::string& path) {
    std::ifstream in(path);
    if (!in) die("cannot open " + path);
    Instance t;
    if (!(in >> t.E >> t.R >> t.F >> t.S)) die("truncated .tim header in " + path);
    auto read = [&](std::vector<int32_t>& v, long n) {
        v.resize(n);
        for (long i = 0; i < n; i++)
            if (!(in >> v[i])) die("truncated .tim body in " + path);
    };
    read(t.room_size, t.R);
    read(t.student_events, (long)t.S * t.E);
    read(t.room_features, (long)t.R * t.F);
    read(t.event_features, (long)t.E * t.F);
    return t;
}

// ---------------------------------------------------------------- JSON
// jsoncpp StreamWriterBuilder with indentation "" (ga.cpp:170-171): compact,
// keys in std::map order, doubles "%.17g" (jsoncpp.cpp:4036-4068).
struct Json {
    enum Kind { Int, Bool, Real, Arr, Obj } kind = Obj;
    long i = 0;
    double d = 0;
    std::vector<long> arr;
    std::map<std::string, Json> obj;
    static Json I(long v) { Json j; j.kind = Int; j.i = v; return j; }
    static Json B(bool v) { Json j; j.kind = Bool; j.i = v; return j; }
    static Json D(double v) { Json j; j.kind = Real; j.d = v; return j; }
    static Json A(std::vector<long> v) { Json j; j.kind = Arr; j.arr = std::move(v); return j; }
    std::string str() const {
        char buf[40];
        switch (kind) {
            case Int: return std::to_string(i);
            case Bool: return i ? "true" : "false";
            case Real:
                if (std::isnan(d)) return "null";
                if (std::isinf(d)) return d < 0 ? "-1e+9999" : "1e+9999";
                std::snprintf(buf, sizeof buf, "%.17g", d);
                return buf;
            case Arr: {
                std::string s = "[";
                for (size_t k = 0; k < arr.size(); k++) s += (k ? "," : "") + std::to_string(arr[k]);
                return s + "]";
            }
            case Obj: {
                std::string s = "{";
                bool first = true;
                for (auto& kvp : obj) {
                    s += (first ? "\"" : ",\"") + kvp.first + "\":" + kvp.second.str();
                    first = false;
                }
                return s + "}";
            }
        }
        return "";
    }
};

Json wrap(const char* key, Json inner) {
    Json j;
    j.obj[key] = std::move(inner);
    return j;
}

// The four JSON line kinds of ga.cpp, shared by the driver and --replay-log.
// setCurrentCost state (ga.cpp:57-58, reset by beginTry :163-167) and decision (:203-228):
// feasible pop[0] logs when its scv differs from the last logged best,
// infeasible when hcv*1e6+scv is lower.
struct CostState {
    long best_scv = INT_MAX, best_eval = INT_MAX;
    bool offer(bool feasible, int scv, int hcv, long& entry) {
        if (feasible) {
            if (scv == best_scv) return false;
            best_scv = best_eval = entry = scv;
            return true;
        }
        const long ev = (long)hcv * 1000000 + scv;
        if (ev >= best_eval) return false;
        best_eval = entry = ev;
        return true;
    }
};

Json log_line(long best, int proc, int thread, double t) {
    Json e;
    e.obj["best"] = Json::I(best);
    e.obj["procID"] = Json::I(proc);
    e.obj["threadID"] = Json::I(thread);
    e.obj["time"] = Json::D(std::max(0.0, t));
    return wrap("logEntry", e);
}

// setGlobalCost (ga.cpp:234-257), printed by rank 0
Json run_best_line(bool feasible, long total_best) {
    Json r;
    r.obj["feasible"] = Json::B(feasible);
    r.obj["totalBest"] = Json::I(total_best);
    return wrap("runEntry", r);
}

// endTry (ga.cpp:169-197); threadID is the global tid, 0 outside the parallel region
Json solution_line(bool feasible, int scv, int hcv, const std::vector<uint8_t>& sl, const std::vector<uint8_t>& rm,
                   int proc, double t) {
    Json s;
    s.obj["feasible"] = Json::B(feasible);
    s.obj["procID"] = Json::I(proc);
    s.obj["threadID"] = Json::I(0);
    s.obj["totalTime"] = Json::D(t);
    if (feasible) {
        s.obj["totalBest"] = Json::I(scv);
        s.obj["timeslots"] = Json::A(std::vector<long>(sl.begin(), sl.end()));
        s.obj["rooms"] = Json::A(std::vector<long>(rm.begin(), rm.end()));
    } else {
        s.obj["totalBest"] = Json::I((long)hcv * 1000000 + scv);
    }
    return wrap("solution", s);
}

// main's closing runEntry (ga.cpp:603-609)
Json run_final_line(int procs, int threads, double t) {
    Json r;
    r.obj["procsNum"] = Json::I(procs);
    r.obj["threadsNum"] = Json::I(threads);
    r.obj["totalTime"] = Json::D(t);
    return wrap("runEntry", r);
}

// ttga-ga --replay-log FILE: the lines one island prints when its pop[0] takes
// the given values in turn (no GPU involved; tests/test_json_parity.py checks
// them against the reference's own ga.cpp + jsoncpp). FILE: "proc threads n E",
// n lines "feasible scv hcv tid", then the last member's E slots and E rooms.
// Times print as 0 (the last runEntry: 0.5).
int replay_log(const char* path) {
    std::ifstream in(path);
    if (!in) die(std::string("cannot open ") + path);
    int proc = 0, threads = 1, n = 0, E = 0;
    if (!(in >> proc >> threads >> n >> E) || n < 1 || E < 0) die("bad replay header");
    CostState cs;
    int f = 0, scv = 0, hcv = 0, tid = 0;
    for (int i = 0; i < n; i++) {
        if (!(in >> f >> scv >> hcv >> tid)) die("truncated replay file");
        long entry = 0;
        if (cs.offer(f != 0, scv, hcv, entry)) std::cout << log_line(entry, proc, tid, 0.0).str() << "\n";
    }
    std::vector<uint8_t> sl(E), rm(E);
    for (int e = 0; e < E; e++) { int v; in >> v; sl[e] = (uint8_t)v; }
    for (int e = 0; e < E; e++) { int v; in >> v; rm[e] = (uint8_t)v; }
    if (!in) die("truncated replay file");
    if (proc == 0) std::cout << run_best_line(f != 0, f ? scv : (long)hcv * 1000000 + scv).str() << "\n";
    std::cout << solution_line(f != 0, scv, hcv, sl, rm, proc, 0.0).str() << "\n";
    std::cout << run_final_line(1, threads, 0.5).str() << std::endl;
    return 0;
}

// --report (ttga/report.py population_report + report_line) from the host copies
// of tt_eval_parts' parts[N][6] and tt_slot_histogram's hist[E][45]
Json report_line(const std::vector<int32_t>& parts, const std::vector<int32_t>& hist, int N, int E, int proc,
                 int island) {
    static const char* const kNames[TT_NUM_PARTS] = {"room_pairs", "corr_pairs", "unsuitable",
                                                     "last_slot", "consecutive", "single_class"};
    long sum[TT_NUM_PARTS] = {0}, nonzero[TT_NUM_PARTS] = {0}, valid = 0, feasible = 0;
    for (int i = 0; i < N; i++) {
        const int32_t* r = &parts[(size_t)i * TT_NUM_PARTS];
        if (r[0] < 0) continue;
        valid++;
        feasible += r[0] + r[1] + r[2] == 0;
        for (int k = 0; k < TT_NUM_PARTS; k++) { sum[k] += r[k]; nonzero[k] += r[k] != 0; }
    }
    long long differing = 0;
    for (int e = 0; e < E; e++) {
        long long n = 0, sq = 0;
        for (int t = 0; t < TT_NUM_SLOTS; t++) {
            const long long h = hist[(size_t)e * TT_NUM_SLOTS + t];
            n += h;
            sq += h * h;
        }
        differing += n * n - sq;
    }
    Json best, psum, pnz, popu, div, rep;
    for (int k = 0; k < TT_NUM_PARTS; k++) {
        best.obj[kNames[k]] = Json::I(parts[k]);
        psum.obj[kNames[k]] = Json::I(sum[k]);
        pnz.obj[kNames[k]] = Json::I(nonzero[k]);
    }
    popu.obj["size"] = Json::I(N);
    popu.obj["feasible"] = Json::I(feasible);
    popu.obj["invalid"] = Json::I(N - valid);
    popu.obj["sum"] = psum;
    popu.obj["nonzero"] = pnz;
    div.obj["events"] = Json::I(E);
    div.obj["size"] = Json::I(N);
    div.obj["pairs_differing"] = Json::I((long)(differing / 2));
    rep.obj["best"] = best;
    rep.obj["population"] = popu;
    rep.obj["diversity"] = div;
    rep.obj["procID"] = Json::I(proc);
    rep.obj["island"] = Json::I(island);
    return wrap("report", rep);
}

// --unique (ttga/ga.py unique_line)
Json unique_line(long children, long dropped, long distinct, int proc, int island) {
    Json u;
    u.obj["children"] = Json::I(children);
    u.obj["dropped"] = Json::I(dropped);
    u.obj["distinct"] = Json::I(distinct);
    u.obj["procID"] = Json::I(proc);
    u.obj["island"] = Json::I(island);
    return wrap("unique", u);
}

// ---------------------------------------------------------------- islands
struct Pop {
    int n = 0, E = 0;
    uint8_t *slot = nullptr, *room = nullptr, *feasible = nullptr;
    int32_t *hcv = nullptr, *scv = nullptr, *penalty = nullptr;
    void alloc(int n_, int E_) {
        n = n_; E = E_;
        check_hip(hipMalloc(&slot, (size_t)n * E), "hipMalloc");
        check_hip(hipMalloc(&room, (size_t)n * E), "hipMalloc");
        check_hip(hipMalloc(&feasible, (size_t)n), "hipMalloc");
        check_hip(hipMalloc(&hcv, 4 * (size_t)n), "hipMalloc");
        check_hip(hipMalloc(&scv, 4 * (size_t)n), "hipMalloc");
        check_hip(hipMalloc(&penalty, 4 * (size_t)n), "hipMalloc");
        check_hip(hipMemset(slot, 0, (size_t)n * E), "hipMemset");
        check_hip(hipMemset(room, 0, (size_t)n * E), "hipMemset");
    }
    void release() {
        for (void* p : {(void*)slot, (void*)room, (void*)feasible, (void*)hcv, (void*)scv, (void*)penalty})
            if (p) (void)hipFree(p);
    }
};

struct Member { bool feasible; int scv, hcv, penalty; };

class Output {
public:
    explicit Output(std::ostream& os) : os_(os) {}
    void line(const Json& j) {
        std::lock_guard<std::mutex> g(mu_);
        os_ << j.str() << std::endl;
    }
private:
    std::ostream& os_;
    std::mutex mu_;
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// A stage's per-row outputs, appended call after call on the device and read once at the
// end, so that no generation waits for them: K int32 columns of `cap` rows (column k at
// col(k)) and, where asked for, a uint8 column. A stage that is off never allocates its log.
template <int K>
struct RunLog {
    struct Host { std::vector<int32_t> col[K]; std::vector<uint8_t> bytes; long rows = 0; };
    int32_t* data = nullptr;
    uint8_t* bytes = nullptr;
    long cap = 0, used = 0;
    const char* what = "";                            // of reserve()'s "more ... than planned for"

    void alloc(long rows, const char* what_, bool with_bytes = false) {
        cap = rows;
        what = what_;
        check_hip(hipMalloc(&data, 4 * (size_t)K * cap), "hipMalloc");
        if (with_bytes) check_hip(hipMalloc(&bytes, (size_t)cap), "hipMalloc");
    }
    int32_t* col(int k) const { return data + k * cap; }
    // room for the next n rows: their offset
    long reserve(long n) {
        if (used + n > cap) die(std::string("more ") + what + " than planned for");
        used += n;
        return used - n;
    }
    // the rows so far on the host, once the streams that wrote them have finished
    Host fetch() const {
        Host h;
        h.rows = used;
        for (int k = 0; k < K; k++) {
            h.col[k].resize(used);
            if (used) check_hip(hipMemcpy(h.col[k].data(), col(k), 4 * (size_t)used, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        if (bytes) {
            h.bytes.resize(used);
            if (used) check_hip(hipMemcpy(h.bytes.data(), bytes, (size_t)used, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        return h;
    }
    void release() {
        if (data) (void)hipFree(data);
        if (bytes) (void)hipFree(bytes);
    }
};

struct Island {
    int id = 0, device = 0, N = 0, C = 0, E = 0, max_steps = 0;
    long seed = 0;
    double p1 = 1, p2 = 1, p3 = 0, p_cross = 0.8, p_mut = 0.5;
    tt_problem* tp = nullptr;
    hipStream_t st = nullptr;
    Pop pop, child;
    int64_t *rng_init = nullptr, *rng_child = nullptr;
    uint8_t* flags = nullptr;
    void* work = nullptr;
    int32_t* order = nullptr;                         // LPT dispatch order (C >= kLptMinChildren)
    static constexpr int kLptMinChildren = 4096;      // as ttga.ga.Island
    // migrants (ga.cpp:318-335): slot[E] room[E] hcv scv penalty feasible
    uint8_t *send_best = nullptr, *send_second = nullptr, *recv_buf = nullptr;
    size_t migrant_bytes = 0;
    CostState cost;                                   // setCurrentCost state (ga.cpp:163-167)
    // the generation's pipeline (ttga.ga.Island): part j of the child rows [off, off + n)
    // on stream s with its own work buffer; every population operation (breed or replace)
    // follows the previous one, so sub-batch h is bred after the replacement of h - parts
    // and h - parts + 1 is replaced after the breed of h. parts == 1 (no --stagger) is the
    // batch schedule: part[0] = {0, C, st, its work buffer}, each sub-batch replaced behind its own
    // search, and neither ev_op nor another stream or work buffer exists
    int parts = 1;
    // lw_work, lw_gain: --lahc-walkers' work buffer and walker gains [rows][K] of the part's stream
    struct Part {
        int off = 0, n = 0;
        hipStream_t s = nullptr;
        void* work = nullptr;
        void* lw_work = nullptr;
        int32_t* lw_gain = nullptr;
    };
    std::vector<Part> part;
    hipEvent_t ev_op = nullptr;                       // behind the last population operation (parts > 1)
    hipStream_t op_stream = nullptr;                  // the stream that operation ran on
    std::vector<int> pending;                         // parts searched, not yet replaced (breed order)
    int last_replace = 0;
    Stages stage;
    // --unique: every replacement is tt_ga_replace_unique; replacement number r leaves its
    // kept count in row r of kept_log (the initial sort, C = 0, has none); children = those
    // that went through a replacement
    uint8_t* keep = nullptr;                          // [C], part j's flags at keep + off
    RunLog<1> kept_log;
    long children = 0;
    RunLog<1> chain_log;                              // --kempe: every child's chain length
    RunLog<2> swap_log;                               // --slot-swap: every searched row's gain and passes
    RunLog<2> lahc_log;                               // --lahc: every searched row's gain, accepted and feasible flag
    // --lahc-kempe: every searched row's lk_width() counts, row-major (five; seven under
    // --lahc-kempe-rooms augment and under --lahc-walkers, whose call writes seven)
    RunLog<7> lk_log;
    int lk_width() const { return stage.lahc_kempe_augment || stage.lahc_walkers > 1 ? 7 : 5; }
    RunLog<2> lw_log;                                 // --lahc-walkers: every searched row's winner and walker 0's gain
    RunLog<2> m1_log;                                 // --move1-descent: every searched row's gain and passes
    RunLog<2> cx_log;                                 // --crossover guided: every child's cost, repaired and flags
    int32_t* ev_order = nullptr;                      // event_order()'s, once computed

    size_t work_bytes(int n) const {
        return std::max<size_t>(stage.unique ? tt_ga_unique_work_bytes(N, n, E) : tt_ga_work_bytes(N, E), 16);
    }

    // tt_greedy_order's event order (--init greedy, --crossover guided): computed on first
    // use, finished on return, and kept for the island's life
    const int32_t* event_order() {
        if (!ev_order) {
            void* scratch = nullptr;
            check_hip(hipMalloc(&ev_order, 4 * (size_t)E), "hipMalloc");
            check_hip(hipMalloc(&scratch, tt_greedy_work_bytes(tp)), "hipMalloc");
            check_tt(tt_greedy_order(tp, ev_order, scratch, st), "tt_greedy_order");
            check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
            check_hip(hipFree(scratch), "hipFree");
        }
        return ev_order;
    }

    void setup(const Instance& inst, long replacements) {
        check_hip(hipSetDevice(device), "hipSetDevice");
        check_tt(tt_problem_create(inst.E, inst.R, inst.F, inst.S, inst.room_size.data(), inst.student_events.data(),
                                   inst.room_features.data(), inst.event_features.data(), device, &tp),
                 "tt_problem_create");
        E = inst.E;
        check_hip(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
        pop.alloc(N, E);
        child.alloc(C, E);
        std::vector<int64_t> s(N + C);
        for (int k = 0; k < N + C; k++) s[k] = std::labs(seed) + 1 + k;     // ttga/ga.py stream_seeds
        check_hip(hipMalloc(&rng_init, 8 * (size_t)N), "hipMalloc");
        check_hip(hipMalloc(&rng_child, 8 * (size_t)C), "hipMalloc");
        check_hip(hipMemcpy(rng_init, s.data(), 8 * (size_t)N, hipMemcpyHostToDevice), "hipMemcpy");
        check_hip(hipMemcpy(rng_child, s.data() + N, 8 * (size_t)C, hipMemcpyHostToDevice), "hipMemcpy");
        check_hip(hipMalloc(&flags, (size_t)C), "hipMalloc");
        if (C >= kLptMinChildren) check_hip(hipMalloc(&order, 4 * (size_t)C), "hipMalloc");
        const long bred = std::max(replacements / parts * C, 1L);      // generations x children
        if (stage.unique) {
            check_hip(hipMalloc(&keep, (size_t)C), "hipMalloc");
            kept_log.alloc(std::max(replacements, 1L), "replacements");
        }
        if (stage.kempe > 0) chain_log.alloc(bred, "Kempe moves");
        if (stage.slot_swap > 0) swap_log.alloc(N + bred, "timeslot-swap rows");          // the members too
        if (stage.lahc > 0) lahc_log.alloc(N + bred, "late-acceptance rows", true);       // the members too
        if (stage.lahc_kempe > 0) lk_log.alloc(N + bred, "late-acceptance rows");
        if (stage.lahc_walkers > 1) lw_log.alloc(N + bred, "late-acceptance rows");
        if (stage.move1_descent > 0) m1_log.alloc(N + bred, "single-event descent rows");  // the members too
        if (stage.guided) {
            cx_log.alloc(bred, "guided crossovers", true);
            event_order();                            // before any part's stream breeds in it
        }
        migrant_bytes = 2 * (size_t)E + 13;
        check_hip(hipMalloc(&send_best, migrant_bytes), "hipMalloc");
        check_hip(hipMalloc(&send_second, migrant_bytes), "hipMalloc");
        check_hip(hipMalloc(&recv_buf, 2 * migrant_bytes), "hipMalloc");
        if (parts > 1) check_hip(hipEventCreateWithFlags(&ev_op, hipEventDisableTiming), "hipEventCreate");
        op_stream = st;
        part.assign(parts, Part{0, 0, st, work});
        for (int j = 0, off = 0; j < parts; j++) {              // numpy.array_split's sizes
            part[j].off = off;
            part[j].n = C / parts + (j < C % parts ? 1 : 0);
            off += part[j].n;
            if (j > 0) check_hip(hipStreamCreateWithFlags(&part[j].s, hipStreamNonBlocking), "hipStreamCreate");
            check_hip(hipMalloc(&part[j].work, work_bytes(part[j].n)), "hipMalloc");
            if (stage.lahc_walkers > 1) {               // once: the first part's stream walks the members too
                const int rows = j == 0 ? std::max(part[j].n, N) : part[j].n;
                check_hip(hipMalloc(&part[j].lw_work, std::max<size_t>(tt_lahc_multi_work_bytes(tp, rows, stage.lahc_walkers), 16)),
                          "hipMalloc");
                check_hip(hipMalloc(&part[j].lw_gain, 4 * (size_t)rows * stage.lahc_walkers), "hipMalloc");
            }
        }
        work = part[0].work;
    }

    // All cross-stream ordering: what s runs next comes after the last population
    // operation (nothing to do when that ran on s, as it always did with one part) ...
    void wait_op(hipStream_t s) {
        if (s != op_stream) check_hip(hipStreamWaitEvent(s, ev_op, 0), "hipStreamWaitEvent");
    }

    // ... and a population operation (breed, replace, or a write of the population by
    // the caller: the initial broadcast, the migrants) has just been enqueued on s
    void wrote_population(hipStream_t s) {
        op_stream = s;
        if (parts > 1) check_hip(hipEventRecord(ev_op, s), "hipEventRecord");
    }

    void evaluate(Pop& p, hipStream_t s = nullptr) {
        check_tt(tt_eval(tp, p.slot, p.room, p.n, p.hcv, p.scv, p.feasible, p.penalty, s ? s : st), "tt_eval");
    }

    // ga.cpp:429-434 for every member, then the population is sorted
    void initialize() {
        if (stage.greedy)
            check_tt(tt_greedy_init(tp, event_order(), rng_init, pop.slot, pop.room, N, st), "tt_greedy_init");
        else
            check_tt(tt_random_init(tp, rng_init, pop.slot, pop.room, N, st), "tt_random_init");
        check_tt(tt_local_search_eval(tp, pop.slot, pop.room, rng_init, N, max_steps, p1, p2, p3, nullptr, pop.hcv,
                                      pop.scv, pop.feasible, pop.penalty, st),
                 "tt_local_search_eval");
        if (stage.slot_swap > 0) swap_slots(pop, st);
        if (stage.lahc > 0) late_acceptance(pop, rng_init, st);
        if (stage.move1_descent > 0) descend_move1(pop, st);
        if (stage.unique)
            check_tt(tt_ga_replace_unique(tp, pop.slot, pop.room, pop.hcv, pop.scv, pop.feasible, pop.penalty, N,
                                          pop.slot, pop.room, pop.hcv, pop.scv, pop.feasible, pop.penalty, 0, nullptr,
                                          nullptr, 0, work, st),
                     "tt_ga_replace_unique");
        else
            check_tt(tt_ga_replace(tp, pop.slot, pop.room, pop.hcv, pop.scv, pop.feasible, pop.penalty, N, pop.slot,
                                   pop.room, pop.hcv, pop.scv, pop.feasible, pop.penalty, 0, work, st),
                     "tt_ga_replace");
        wrote_population(st);
    }

    // children rows [off, off + n) as a population view
    Pop child_rows(int off, int n) const {
        Pop v;
        v.n = n; v.E = E;
        v.slot = child.slot + (size_t)off * E; v.room = child.room + (size_t)off * E;
        v.feasible = child.feasible + off; v.hcv = child.hcv + off; v.scv = child.scv + off;
        v.penalty = child.penalty + off;
        return v;
    }

    // every part's stream (part 0's is st) has finished: the logs can be read
    void finish() {
        for (const Part& p : part) check_hip(hipStreamSynchronize(p.s), "hipStreamSynchronize");
    }

    // a log's rows with every sub-batch replaced
    template <int K>
    typename RunLog<K>::Host read(const RunLog<K>& log) {
        flush();
        finish();
        return log.fetch();
    }

    // breed n children into rows [off, off + n) on stream s
    void breed(int off, int n, hipStream_t s) {
        Pop c = child_rows(off, n);
        if (stage.guided) {
            const long at = cx_log.reserve(n);
            check_tt(tt_ga_breed_guided(tp, pop.slot, pop.room, pop.penalty, N, event_order(), rng_child + off, n,
                                        p_cross, p_mut, 1, stage.cx_repair, c.slot, c.room, flags + off,
                                        cx_log.col(0) + at, cx_log.col(1) + at, s),
                     "tt_ga_breed_guided");
            check_hip(hipMemcpyAsync(cx_log.bytes + at, flags + off, (size_t)n, hipMemcpyDeviceToDevice, s),
                      "hipMemcpyAsync");
            return;
        }
        check_tt(tt_ga_breed(tp, pop.slot, pop.room, pop.penalty, N, rng_child + off, n, p_cross, p_mut, 1, c.slot,
                             c.room, flags + off, s),
                 "tt_ga_breed");
    }

    // the --crossover guided line (ttga/ga.py crossover_line)
    Json crossover_report() {
        const auto h = read(cx_log);
        long crossed = 0, clean = 0, total = 0, repaired = 0;
        for (long i = 0; i < h.rows; i++) {
            const bool x = (h.bytes[i] & 1) != 0;
            crossed += x;
            clean += x && h.col[0][i] == 0;
            total += h.col[0][i];
            repaired += h.col[1][i];
        }
        Json k;
        k.obj["children"] = Json::I(h.rows);
        k.obj["crossed"] = Json::I(crossed);
        k.obj["clean"] = Json::I(clean);
        k.obj["meanCost"] = Json::D(crossed ? (double)total / (double)crossed : 0.0);
        k.obj["repaired"] = Json::I(repaired);
        return wrap("crossover", k);
    }

    // --kempe: the Kempe-chain move on rows [off, off + n) on s, from the children's own streams
    void kempe_move(int off, int n, hipStream_t s) {
        Pop c = child_rows(off, n);
        check_tt(tt_kempe_move(tp, c.slot, c.room, rng_child + off, n, stage.kempe, stage.kempe_max_chain,
                               chain_log.col(0) + chain_log.reserve(n), s),
                 "tt_kempe_move");
    }

    // the --kempe line (ttga/ga.py kempe_line)
    Json kempe_report() {
        const auto h = read(chain_log);
        long moved = 0, rejected = 0, events = 0;
        for (int32_t v : h.col[0]) {
            moved += v > 0;
            rejected += v < 0;
            if (v > 0) events += v;
        }
        Json k;
        k.obj["children"] = Json::I(h.rows);
        k.obj["moved"] = Json::I(moved);
        k.obj["rejected"] = Json::I(rejected);
        k.obj["meanChain"] = Json::D(moved ? (double)events / (double)moved : 0.0);
        return wrap("kempe", k);
    }

    // --slot-swap: the timeslot-swap descent on the searched rows r on s, behind their search
    // and evaluation; their scv and penalty are lowered in place
    void swap_slots(const Pop& r, hipStream_t s) {
        const long at = swap_log.reserve(r.n);
        check_tt(tt_slot_swap(tp, r.slot, r.n, stage.slot_swap, r.scv, r.penalty, swap_log.col(0) + at,
                              swap_log.col(1) + at, nullptr, s),
                 "tt_slot_swap");
    }

    // the --slot-swap line (ttga/ga.py slot_swap_line)
    Json slot_swap_report() {
        const auto h = read(swap_log);
        long improved = 0, passes = 0, total = 0;
        for (long i = 0; i < h.rows; i++) {
            improved += h.col[1][i] > 0;
            passes += h.col[1][i];
            total += h.col[0][i];
        }
        Json k;
        k.obj["rows"] = Json::I(h.rows);
        k.obj["improved"] = Json::I(improved);
        k.obj["gain"] = Json::I(total);
        k.obj["meanPasses"] = Json::D(improved ? (double)passes / (double)improved : 0.0);
        return wrap("slotSwap", k);
    }

    // --move1-descent: the single-event steepest descent on the searched rows r on s, behind
    // their search, evaluation, timeslot swap and walk; their scv and penalty are lowered in place
    void descend_move1(const Pop& r, hipStream_t s) {
        const long at = m1_log.reserve(r.n);
        check_tt(tt_move1_descent(tp, r.slot, r.room, r.n, stage.move1_descent, r.scv, r.penalty, m1_log.col(0) + at,
                                  m1_log.col(1) + at, s),
                 "tt_move1_descent");
    }

    // the --move1-descent line (ttga/ga.py move1_descent_line)
    Json move1_descent_report() {
        const auto h = read(m1_log);
        long improved = 0, passes = 0, total = 0;
        for (long i = 0; i < h.rows; i++) {
            improved += h.col[1][i] > 0;
            passes += h.col[1][i];
            total += h.col[0][i];
        }
        Json k;
        k.obj["rows"] = Json::I(h.rows);
        k.obj["improved"] = Json::I(improved);
        k.obj["gain"] = Json::I(total);
        k.obj["meanPasses"] = Json::D(improved ? (double)passes / (double)improved : 0.0);
        return wrap("move1Descent", k);
    }

    // --lahc: the late-acceptance walk of the searched rows r (streams g) on s, behind their
    // search, evaluation and timeslot swap; their scv and penalty are lowered in place
    void late_acceptance(const Pop& r, int64_t* g, hipStream_t s) {
        const long at = lahc_log.reserve(r.n);
        if (stage.lahc_walkers > 1) {
            // the walk the branches below would call: without chains p_kempe 0 and room_rule 0
            const Part* q = &part[0];
            for (const Part& x : part)
                if (x.s == s) q = &x;
            const int K = stage.lahc_walkers;
            if (stage.lahc_kempe > 0) lk_log.reserve(r.n);
            const long aw = lw_log.reserve(r.n);        // row for row with lahc_log
            check_tt(tt_lahc_multi(tp, r.slot, r.room, g, r.n, K, stage.lahc, stage.lahc_history, stage.lahc_swap,
                                   stage.lahc_kempe, stage.lahc_kempe_max_chain, stage.lahc_kempe_augment ? 1 : 0, r.scv,
                                   r.penalty, lahc_log.col(0) + at, lahc_log.col(1) + at, nullptr,
                                   stage.lahc_kempe > 0 ? lk_log.data + 7 * at : nullptr, lw_log.col(0) + aw, q->lw_gain,
                                   q->lw_work, s),
                     "tt_lahc_multi");
            check_hip(hipMemcpy2DAsync(lw_log.col(1) + aw, 4, q->lw_gain, 4 * (size_t)K, 4, (size_t)r.n,
                                       hipMemcpyDeviceToDevice, s),
                      "hipMemcpy2DAsync");
        } else if (stage.lahc_kempe > 0 && stage.lahc_kempe_augment) {
            lk_log.reserve(r.n);                      // row for row with lahc_log
            check_tt(tt_lahc_kempe_aug(tp, r.slot, r.room, g, r.n, stage.lahc, stage.lahc_history, stage.lahc_swap,
                                       stage.lahc_kempe, stage.lahc_kempe_max_chain, 1, r.scv, r.penalty,
                                       lahc_log.col(0) + at, lahc_log.col(1) + at, nullptr, lk_log.data + 7 * at, s),
                     "tt_lahc_kempe_aug");
        } else if (stage.lahc_kempe > 0) {
            lk_log.reserve(r.n);                      // row for row with lahc_log
            check_tt(tt_lahc_kempe(tp, r.slot, r.room, g, r.n, stage.lahc, stage.lahc_history, stage.lahc_swap,
                                   stage.lahc_kempe, stage.lahc_kempe_max_chain, r.scv, r.penalty, lahc_log.col(0) + at,
                                   lahc_log.col(1) + at, nullptr, lk_log.data + 5 * at, s),
                     "tt_lahc_kempe");
        } else {
            check_tt(tt_lahc(tp, r.slot, r.room, g, r.n, stage.lahc, stage.lahc_history, stage.lahc_swap, r.scv,
                             r.penalty, lahc_log.col(0) + at, lahc_log.col(1) + at, nullptr, s),
                     "tt_lahc");
        }
        check_hip(hipMemcpyAsync(lahc_log.bytes + at, r.feasible, (size_t)r.n, hipMemcpyDeviceToDevice, s),
                  "hipMemcpyAsync");
    }

    // the --lahc line (ttga/ga.py lahc_line)
    Json lahc_report() {
        const auto h = read(lahc_log);
        long searched = 0, improved = 0, accepted = 0, total = 0;
        for (long i = 0; i < h.rows; i++) {
            searched += h.bytes[i] != 0;
            improved += h.col[0][i] > 0;
            accepted += h.col[1][i];
            total += h.col[0][i];
        }
        Json k;
        k.obj["rows"] = Json::I(h.rows);
        k.obj["searched"] = Json::I(searched);
        k.obj["improved"] = Json::I(improved);
        k.obj["accepted"] = Json::I(accepted);
        k.obj["gain"] = Json::I(total);
        return wrap("lahc", k);
    }

    // the --lahc-kempe line (ttga/ga.py lahc_kempe_line)
    Json lahc_kempe_report() {
        flush();
        finish();
        const int width = lk_width();
        std::vector<int32_t> h((size_t)width * (size_t)lk_log.used);
        if (lk_log.used) check_hip(hipMemcpy(h.data(), lk_log.data, 4 * h.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        long sum[7] = {0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < h.size(); i++) sum[i % width] += h[i];
        Json k;
        k.obj["tried"] = Json::I(sum[0]);
        k.obj["capped"] = Json::I(sum[1]);
        k.obj["noRoom"] = Json::I(sum[2]);
        k.obj["accepted"] = Json::I(sum[3]);
        k.obj["meanChain"] = Json::D(sum[3] ? (double)sum[4] / (double)sum[3] : 0.0);
        if (stage.lahc_kempe_augment) {
            k.obj["rescued"] = Json::I(sum[5]);
            k.obj["displaced"] = Json::I(sum[6]);
        }
        return wrap("lahcKempe", k);
    }

    // the --lahc-walkers line (ttga/ga.py lahc_walkers_line); lahc_log and lw_log go row for row
    Json lahc_walkers_report() {
        const auto h = read(lahc_log);
        const auto w = read(lw_log);
        long rows = 0, total = 0, first = 0, later = 0;
        for (long i = 0; i < h.rows && i < w.rows; i++) {
            rows += h.bytes[i] != 0;
            total += h.col[0][i];
            first += w.col[1][i];
            later += w.col[0][i] > 0;
        }
        Json k;
        k.obj["rows"] = Json::I(rows);
        k.obj["walkers"] = Json::I(stage.lahc_walkers);
        k.obj["gain"] = Json::I(total);
        k.obj["gainFirst"] = Json::I(first);
        k.obj["winnerLater"] = Json::I(later);
        return wrap("lahcWalkers", k);
    }

    // LPT order (C >= kLptMinChildren), localSearch and evaluation of rows [off, off + n) on s
    // (the search and the evaluation in one launch: ga.cpp:574-575)
    void search(int off, int n, hipStream_t s, void* w) {
        Pop c = child_rows(off, n);
        const int32_t* ord = nullptr;
        if (order) {
            // longest-expected first: the children's hcv before the search, descending
            // (a generation's search launch ends with its slowest children); same results
            evaluate(c, s);
            check_tt(tt_lpt_order(tp, c.hcv, n, order + off, w, s), "tt_lpt_order");
            ord = order + off;
        }
        check_tt(tt_local_search_eval(tp, c.slot, c.room, rng_child + off, n, max_steps, p1, p2, p3, ord, c.hcv, c.scv,
                                      c.feasible, c.penalty, s),
                 "tt_local_search_eval");
    }

    void replace(int off, int n, hipStream_t s, void* w) {
        Pop c = child_rows(off, n);
        if (stage.unique) {
            check_tt(tt_ga_replace_unique(tp, pop.slot, pop.room, pop.hcv, pop.scv, pop.feasible, pop.penalty, N, c.slot,
                                          c.room, c.hcv, c.scv, c.feasible, c.penalty, n, keep + off,
                                          kept_log.col(0) + kept_log.reserve(1), 0, w, s),
                     "tt_ga_replace_unique");
            children += n;
            return;
        }
        check_tt(tt_ga_replace(tp, pop.slot, pop.room, pop.hcv, pop.scv, pop.feasible, pop.penalty, N, c.slot, c.room,
                               c.hcv, c.scv, c.feasible, c.penalty, n, w, s),
                 "tt_ga_replace");
    }

    // the --unique line of the population with every sub-batch replaced: the kept counts
    // of all replacements, and the first occurrences of the genomes
    Json unique_report(int proc, int island) {
        const auto kept = read(kept_log);
        std::vector<int32_t> first(N);
        int32_t* d_first = nullptr;
        void* d_work = nullptr;
        check_hip(hipMalloc(&d_first, 4 * (size_t)N), "hipMalloc");
        check_hip(hipMalloc(&d_work, std::max<size_t>(tt_genome_work_bytes(N, E), 16)), "hipMalloc");
        check_tt(tt_genome_first(tp, pop.slot, pop.room, N, d_first, 0, d_work, st), "tt_genome_first");
        check_hip(hipMemcpyAsync(first.data(), d_first, 4 * (size_t)N, hipMemcpyDeviceToHost, st), "hipMemcpy");
        check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
        (void)hipFree(d_first);
        (void)hipFree(d_work);
        long kept_sum = 0, distinct = 0;
        for (int32_t v : kept.col[0]) kept_sum += v;
        for (int i = 0; i < N; i++) distinct += first[i] == i;
        return unique_line(children, children - kept_sum, distinct, proc, island);
    }

    // one generation of C children (ga.cpp:543-585): each sub-batch in turn
    void step() {
        for (int j = 0; j < parts; j++) advance(j);
    }

    // sub-batch j: bred behind the last population operation; with parts - 1 older
    // sub-batches pending, the oldest is replaced behind that breed; then j is searched
    // (one part: and replaced at once, the sub-batch parts - 1 behind being itself)
    void advance(int j) {
        const Part& p = part[j];
        wait_op(p.s);                                                            // breed(h) after replace(h - parts)
        breed(p.off, p.n, p.s);
        wrote_population(p.s);
        if (!pending.empty() && (int)pending.size() >= parts - 1) replace_oldest();   // replace(h - parts + 1) after breed(h)
        if (stage.kempe > 0) kempe_move(p.off, p.n, p.s);
        search(p.off, p.n, p.s, p.work);
        if (stage.slot_swap > 0) swap_slots(child_rows(p.off, p.n), p.s);
        if (stage.lahc > 0) late_acceptance(child_rows(p.off, p.n), rng_child + p.off, p.s);
        if (stage.move1_descent > 0) descend_move1(child_rows(p.off, p.n), p.s);
        pending.push_back(j);
        if ((int)pending.size() >= parts) replace_oldest();
    }

    void replace_oldest() {
        const int j = pending.front();
        pending.erase(pending.begin());
        const Part& p = part[j];
        wait_op(p.s);
        replace(p.off, p.n, p.s, p.work);
        wrote_population(p.s);
        last_replace = j;
    }

    // replace the pending sub-batches; st then follows the population's last operation
    void flush() {
        while (!pending.empty()) replace_oldest();
        wait_op(st);
    }

    // pop[k]'s fields, read behind the last replacement enqueued (staggered: the
    // pending half-batch stays pending, as ttga.ga.Island.snapshot)
    Member member_now(int k) {
        const hipStream_t s = part[last_replace].s;
        Member m{};
        uint8_t f = 0;
        check_hip(hipMemcpyAsync(&f, pop.feasible + k, 1, hipMemcpyDeviceToHost, s), "hipMemcpy");
        check_hip(hipMemcpyAsync(&m.scv, pop.scv + k, 4, hipMemcpyDeviceToHost, s), "hipMemcpy");
        check_hip(hipMemcpyAsync(&m.hcv, pop.hcv + k, 4, hipMemcpyDeviceToHost, s), "hipMemcpy");
        check_hip(hipMemcpyAsync(&m.penalty, pop.penalty + k, 4, hipMemcpyDeviceToHost, s), "hipMemcpy");
        check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");
        m.feasible = f != 0;
        return m;
    }

    // pop[k]'s fields with every half-batch replaced
    Member member(int k) {
        flush();
        return member_now(k);
    }

    // the reference thread whose replacement put pop[0] in place (ga.cpp:580-585):
    // child c of the last tt_ga_replace (the source position it leaves at
    // tt_ga_work_source_offset in its work buffer), else 0
    int best_thread(bool after_step) {
        if (!after_step) return 0;
        const Part& p = part[last_replace];
        int32_t src = 0;
        check_hip(hipMemcpyAsync(&src, (const uint8_t*)p.work + tt_ga_work_source_offset(N, E), 4,
                                 hipMemcpyDeviceToHost, p.s),
                  "hipMemcpy");
        check_hip(hipStreamSynchronize(p.s), "hipStreamSynchronize");
        // the child's source word: N - n + c from tt_ga_replace, N + c from tt_ga_replace_unique
        const long k = stage.unique ? N : N - p.n, end = stage.unique ? N + p.n : N;
        return src >= k && src < end ? (int)(p.off + src - k) : 0;
    }

    // setCurrentCost (ga.cpp:203-228) on pop[0] as the last replacement left it
    void log_cost(Output& out, std::chrono::steady_clock::time_point t0, int thread) {
        const Member m = member_now(0);
        long entry = 0;
        if (cost.offer(m.feasible, m.scv, m.hcv, entry)) out.line(log_line(entry, id, thread, seconds_since(t0)));
    }

    // the --report line of the population with every sub-batch replaced
    Json report(int proc, int island) {
        flush();
        int32_t *d_parts = nullptr, *d_hist = nullptr;
        std::vector<int32_t> parts((size_t)N * TT_NUM_PARTS), hist((size_t)E * TT_NUM_SLOTS);
        check_hip(hipMalloc(&d_parts, 4 * parts.size()), "hipMalloc");
        check_hip(hipMalloc(&d_hist, 4 * hist.size()), "hipMalloc");
        check_tt(tt_eval_parts(tp, pop.slot, pop.room, N, d_parts, nullptr, st), "tt_eval_parts");
        check_tt(tt_slot_histogram(tp, pop.slot, N, d_hist, st), "tt_slot_histogram");
        check_hip(hipMemcpyAsync(parts.data(), d_parts, 4 * parts.size(), hipMemcpyDeviceToHost, st), "hipMemcpy");
        check_hip(hipMemcpyAsync(hist.data(), d_hist, 4 * hist.size(), hipMemcpyDeviceToHost, st), "hipMemcpy");
        check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
        (void)hipFree(d_parts);
        (void)hipFree(d_hist);
        return report_line(parts, hist, N, E, proc, island);
    }

    // serializeSolutions(k, 1, ...) (ga.cpp:318-342) into send_buf
    void pack(int k, uint8_t* send_buf) {
        auto cp = [&](void* dst, const void* src, size_t n) {
            check_hip(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
        };
        cp(send_buf, pop.slot + (size_t)k * E, E);
        cp(send_buf + E, pop.room + (size_t)k * E, E);
        cp(send_buf + 2 * E, pop.hcv + k, 4);
        cp(send_buf + 2 * E + 4, pop.scv + k, 4);
        cp(send_buf + 2 * E + 8, pop.penalty + k, 4);
        cp(send_buf + 2 * E + 12, pop.feasible + k, 1);
    }

    // deserializeSolution into position pos (ga.cpp:344-368)
    void unpack(int pos, const uint8_t* buf) {
        auto cp = [&](void* dst, const void* src, size_t n) {
            check_hip(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
        };
        cp(pop.slot + (size_t)pos * E, buf, E);
        cp(pop.room + (size_t)pos * E, buf + E, E);
        cp(pop.hcv + pos, buf + 2 * E, 4);
        cp(pop.scv + pos, buf + 2 * E + 4, 4);
        cp(pop.penalty + pos, buf + 2 * E + 8, 4);
        cp(pop.feasible + pos, buf + 2 * E + 12, 1);
        wrote_population(st);                                  // the next breed sees the migrants
    }

    void release() {
        pop.release();
        child.release();
        for (void* p : {(void*)rng_init, (void*)rng_child, (void*)flags, (void*)order, (void*)send_best,
                        (void*)send_second, (void*)recv_buf, (void*)keep, (void*)ev_order})
            if (p) (void)hipFree(p);
        kept_log.release();
        chain_log.release();
        swap_log.release();
        lahc_log.release();
        lk_log.release();
        lw_log.release();
        m1_log.release();
        cx_log.release();
        for (size_t j = 0; j < part.size(); j++) {
            if (part[j].work) (void)hipFree(part[j].work);
            if (part[j].lw_work) (void)hipFree(part[j].lw_work);
            if (part[j].lw_gain) (void)hipFree(part[j].lw_gain);
            if (j > 0 && part[j].s) (void)hipStreamDestroy(part[j].s);
        }
        if (ev_op) (void)hipEventDestroy(ev_op);
        if (st) (void)hipStreamDestroy(st);
        if (tp) tt_problem_destroy(tp);
    }
};

// Reusable barrier for the island threads (the MPI_Barrier calls of ga.cpp:520,538).
class Barrier {
public:
    explicit Barrier(int n) : n_(n) {}
    void wait() {
        std::unique_lock<std::mutex> lk(mu_);
        const long gen = gen_;
        if (++count_ == n_) { count_ = 0; gen_++; cv_.notify_all(); return; }
        cv_.wait(lk, [&] { return gen != gen_; });
    }
private:
    std::mutex mu_;
    std::condition_variable cv_;
    int n_, count_ = 0;
    long gen_ = 0;
};

}  // namespace

int main(int argc, char** argv) {
    const auto t_start = std::chrono::steady_clock::now();
    if (argc == 3 && !std::strcmp(argv[1], "--replay-log")) return replay_log(argv[2]);
    Control ctl = parse_control(argc, argv);
    Output out(std::cout);                       // ga.cpp:60: -o is parsed, output goes to cout
    const Instance inst = read_tim(ctl.input);

    int ndev = 0;
    check_hip(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    const int G = ctl.gpus;
    if (G < 1 || G > ndev) die("--gpus " + std::to_string(G) + " but " + std::to_string(ndev) + " GPU(s) visible");
    const int K = ctl.islands > 0 ? ctl.islands : G;
    if (ctl.pop < 3) die("--pop must be at least 3 (ring migration writes pop[N-1] and pop[N-2])");
    const int N = ctl.pop;
    const int C = std::max(1, std::min(ctl.threads, N));
    const int gens = ctl.generations >= 0 ? ctl.generations : (2001 + C - 1) / C;   // generations 0..2000 (ga.cpp:510)
    if (ctl.rccl && K != G) die("--rccl needs one island per GPU (--islands equal to --gpus)");
    const bool rccl = K == G && (K > 1 || ctl.rccl);   // one island per GPU: RCCL ring; otherwise device copies

    std::vector<Island> isl(K);
    for (int k = 0; k < K; k++) {
        Island& I = isl[k];
        I.id = k; I.device = k % G; I.N = N; I.C = C;
        I.max_steps = max_steps_for(ctl.problem_type);
        I.seed = island_seed(ctl.seed, k);
        I.p1 = ctl.p1; I.p2 = ctl.p2; I.p3 = ctl.p3;
        I.parts = ctl.stagger >= 2 ? std::min(ctl.stagger, C) : 1;
        I.stage = ctl.stage;
    }
    std::vector<ncclComm_t> comms(K, nullptr);
    if (rccl) {
        std::vector<int> devs(K);
        for (int k = 0; k < K; k++) devs[k] = k;
        check_nccl(ncclCommInitAll(comms.data(), K, devs.data()), "ncclCommInitAll");
    }
    Barrier barrier(K);
    std::vector<long> best_value(K, 0);
    std::vector<int> best_feasible(K, 0);
    std::chrono::steady_clock::time_point t_begin;

    auto sync = [](Island& I) { check_hip(hipStreamSynchronize(I.st), "hipStreamSynchronize"); };
    auto run = [&](int k) {
        Island& I = isl[k];
        I.setup(inst, (long)gens * I.parts);
        if (k == 0) I.initialize();
        sync(I);
        barrier.wait();
        // every island starts from island 0's population (ga.cpp:442-464)
        if (rccl) {
            check_nccl(ncclGroupStart(), "ncclGroupStart");
            check_nccl(ncclBroadcast(I.pop.slot, I.pop.slot, (size_t)N * I.E, ncclUint8, 0, comms[k], I.st), "bcast");
            check_nccl(ncclBroadcast(I.pop.room, I.pop.room, (size_t)N * I.E, ncclUint8, 0, comms[k], I.st), "bcast");
            check_nccl(ncclBroadcast(I.pop.hcv, I.pop.hcv, N, ncclInt32, 0, comms[k], I.st), "bcast");
            check_nccl(ncclBroadcast(I.pop.scv, I.pop.scv, N, ncclInt32, 0, comms[k], I.st), "bcast");
            check_nccl(ncclBroadcast(I.pop.penalty, I.pop.penalty, N, ncclInt32, 0, comms[k], I.st), "bcast");
            check_nccl(ncclBroadcast(I.pop.feasible, I.pop.feasible, N, ncclUint8, 0, comms[k], I.st), "bcast");
            check_nccl(ncclGroupEnd(), "ncclGroupEnd");
        } else if (k > 0) {
            const Pop& z = isl[0].pop;
            auto cp = [&](void* dst, const void* src, size_t n) {
                check_hip(hipMemcpyPeerAsync(dst, I.device, src, isl[0].device, n, I.st), "hipMemcpyPeerAsync");
            };
            cp(I.pop.slot, z.slot, (size_t)N * I.E);
            cp(I.pop.room, z.room, (size_t)N * I.E);
            cp(I.pop.hcv, z.hcv, 4 * (size_t)N);
            cp(I.pop.scv, z.scv, 4 * (size_t)N);
            cp(I.pop.penalty, z.penalty, 4 * (size_t)N);
            cp(I.pop.feasible, z.feasible, (size_t)N);
        }
        I.wrote_population(I.st);                     // the shared population
        sync(I);
        barrier.wait();
        if (k == 0) t_begin = std::chrono::steady_clock::now();      // beginTry (ga.cpp:476)
        barrier.wait();
        I.log_cost(out, t_begin, 0);
        const int right = (k + 1) % K, left = (k + K - 1) % K;
        for (int g = 0; g < gens; g++) {
            if ((g + 1) % 100 == 50) {   // ga.cpp:514-540, one migrant each way
                I.flush();                                // staggered: the pending sub-batches replaced first
                I.pack(0, I.send_best);                   // best, then 2nd best (N >= 3: untouched by dir 0)
                I.pack(1, I.send_second);
                sync(I);
                barrier.wait();
                uint8_t* from_left = I.recv_buf;          // dir 0: left's best -> pop[N-1]
                uint8_t* from_right = I.recv_buf + I.migrant_bytes;   // dir 1: right's 2nd best -> pop[N-2]
                if (rccl) {
                    check_nccl(ncclGroupStart(), "ncclGroupStart");
                    check_nccl(ncclSend(I.send_best, I.migrant_bytes, ncclUint8, right, comms[k], I.st), "ncclSend");
                    check_nccl(ncclRecv(from_left, I.migrant_bytes, ncclUint8, left, comms[k], I.st), "ncclRecv");
                    check_nccl(ncclGroupEnd(), "ncclGroupEnd");
                    check_nccl(ncclGroupStart(), "ncclGroupStart");
                    check_nccl(ncclSend(I.send_second, I.migrant_bytes, ncclUint8, left, comms[k], I.st), "ncclSend");
                    check_nccl(ncclRecv(from_right, I.migrant_bytes, ncclUint8, right, comms[k], I.st), "ncclRecv");
                    check_nccl(ncclGroupEnd(), "ncclGroupEnd");
                } else {
                    check_hip(hipMemcpyPeerAsync(from_left, I.device, isl[left].send_best, isl[left].device,
                                                 I.migrant_bytes, I.st), "hipMemcpyPeerAsync");
                    check_hip(hipMemcpyPeerAsync(from_right, I.device, isl[right].send_second, isl[right].device,
                                                 I.migrant_bytes, I.st), "hipMemcpyPeerAsync");
                }
                I.unpack(N - 1, from_left);
                I.unpack(N - 2, from_right);
                sync(I);
                barrier.wait();      // the neighbours' send buffers are free again
            }
            I.step();
            I.log_cost(out, t_begin, I.best_thread(true));
        }
        const Member b = I.member(0);
        best_feasible[k] = b.feasible;
        best_value[k] = b.feasible ? b.scv : (long)b.hcv * 1000000 + b.scv;
    };
    std::vector<std::thread> th;
    for (int k = 0; k < K; k++) th.emplace_back(run, k);
    for (auto& t : th) t.join();

    // setGlobalCost (ga.cpp:234-257): MIN over islands (RCCL all-reduce across GPUs), printed once
    long gmin = *std::min_element(best_value.begin(), best_value.end());
    if (rccl) {
        std::vector<std::thread> red;
        std::vector<int64_t*> dv(K, nullptr);        // hcv * 1e6 + scv can pass 2^31
        for (int k = 0; k < K; k++)
            red.emplace_back([&, k] {
                Island& I = isl[k];
                check_hip(hipSetDevice(I.device), "hipSetDevice");
                check_hip(hipMalloc(&dv[k], 8), "hipMalloc");
                const int64_t v = best_value[k];
                check_hip(hipMemcpy(dv[k], &v, 8, hipMemcpyHostToDevice), "hipMemcpy");
                check_nccl(ncclAllReduce(dv[k], dv[k], 1, ncclInt64, ncclMin, comms[k], I.st), "ncclAllReduce");
                check_hip(hipStreamSynchronize(I.st), "hipStreamSynchronize");
            });
        for (auto& t : red) t.join();
        int64_t v = 0;
        check_hip(hipSetDevice(0), "hipSetDevice");
        check_hip(hipMemcpy(&v, dv[0], 8, hipMemcpyDeviceToHost), "hipMemcpy");
        gmin = v;
        for (int k = 0; k < K; k++) { (void)hipSetDevice(k); (void)hipFree(dv[k]); }
    }
    out.line(run_best_line(best_feasible[0] != 0, gmin));
    // endTry (ga.cpp:169-197) per island
    for (int k = 0; k < K; k++) {
        Island& I = isl[k];
        check_hip(hipSetDevice(I.device), "hipSetDevice");
        const Member b = I.member(0);
        std::vector<uint8_t> sl(I.E), rm(I.E);
        check_hip(hipMemcpy(sl.data(), I.pop.slot, I.E, hipMemcpyDeviceToHost), "hipMemcpy");
        check_hip(hipMemcpy(rm.data(), I.pop.room, I.E, hipMemcpyDeviceToHost), "hipMemcpy");
        out.line(solution_line(b.feasible, b.scv, b.hcv, sl, rm, k, seconds_since(t_begin)));
        if (ctl.stage.guided) out.line(I.crossover_report());
        if (ctl.stage.kempe > 0) out.line(I.kempe_report());
    }
    // then, kind by kind, the lines that every island prints
    auto each_island = [&](bool on, auto line) {
        for (int k = 0; on && k < K; k++) {
            check_hip(hipSetDevice(isl[k].device), "hipSetDevice");
            out.line(line(isl[k], k));
        }
    };
    each_island(ctl.stage.unique, [](Island& I, int k) { return I.unique_report(k, k); });
    each_island(ctl.stage.slot_swap > 0, [](Island& I, int) { return I.slot_swap_report(); });
    each_island(ctl.stage.lahc > 0, [](Island& I, int) { return I.lahc_report(); });
    each_island(ctl.stage.lahc_kempe > 0, [](Island& I, int) { return I.lahc_kempe_report(); });
    each_island(ctl.stage.lahc_walkers > 1, [](Island& I, int) { return I.lahc_walkers_report(); });
    each_island(ctl.stage.move1_descent > 0, [](Island& I, int) { return I.move1_descent_report(); });
    each_island(ctl.report, [](Island& I, int k) { return I.report(k, k); });
    out.line(run_final_line(K, C, seconds_since(t_start)));
    for (int k = 0; k < K; k++) {
        (void)hipSetDevice(isl[k].device);
        isl[k].release();
        if (comms[k]) ncclCommDestroy(comms[k]);
    }
    return 0;
}
