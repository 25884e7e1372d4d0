/* oracle/ref_standins/ref_api.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * extern "C" access to the reference's own SimpleGame and SimpleRaceGame objects.  `make -C oracle ref REFERENCE=<tree>`
 * compiles this file together with the reference's unmodified sources (read in place from <tree>) against the stand-in
 * headers of this directory into oracle/_ref/libxwref.so; tests/_ref.py loads it.  Nothing of the reference is copied here:
 * the calls below are the ones SimulatorInterface makes (simulator_interface.cpp:95-105,126-137), in its order.
 *
 * Threads.  util::thread_local_reng() is per thread and, with FLAGS_simulator_seed != 0, seeded from a process-wide thread
 * counter (simulator_util.cpp:38-55).  xwref_rollout() therefore runs one env on a fresh std::thread, started and joined
 * before it returns, and touches the engine first: while the seed flag is non-zero every rollout is exactly one more counted
 * thread, in call order.  xwref_threads() mirrors the reference's private counter.  Envs made with xwref_create live on the
 * caller's thread and must not draw random numbers: FLAGS_random is refused there. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <thread>
#include <typeindex>
#include <unordered_map>
#include <vector>

#include "simulator.h"
#include "games/simple_game/simple_game_simulator.h"
/* The car (RaceEngine::_car inside SimpleRaceGame::_race) has no public getter.  Access specifiers change neither layout nor
 * symbol names with this compiler, so this translation unit alone reads the class definition with them opened; the reference's
 * own translation units are compiled as they are.  Every standard header the file pulls in is already included above. */
#define private public
#define protected public
#include "games/simple_race/simple_race_simulator.h"
#undef private
#undef protected

DECLARE_int32(simulator_seed);
DECLARE_double(reward_scale);

using simulator::GameSimulator;
using simulator::StatePacket;

namespace {

int g_threads = 0;

struct Env {
    int game;                       /* 0 SimpleGame, 1 SimpleRaceGame */
    GameSimulator* g;
};

[[noreturn]] void die(const char* msg) {
    std::fprintf(stderr, "ref_api: %s\n", msg);
    std::abort();
}

Env* env_create(int game) {
    Env* e = new Env;
    e->game = game;
    if (game == 0) e->g = new simulator::simple_game::SimpleGame();
    else if (game == 1) e->g = new simulator::simple_race::SimpleRaceGame();
    else die("unknown game");
    return e;
}

/* SimulatorInterface::reset_game without a teacher */
void env_reset(Env* e) {
    e->g->reset_game();
    e->g->init_screen();
}

/* SimulatorInterface::take_actions without a teacher; the action travels as the "action" id of a StatePacket */
float env_take_actions(Env* e, int action, int act_rep) {
    StatePacket actions;
    actions.add_buffer_id("action", std::vector<int>({action}));
    float r = 0;
    r += e->g->take_actions(actions, act_rep, false, 0);
    e->g->make_context_screens();
    return r;
}

/* SimulatorInterface::get_state: the FLAGS_context most recent screens, oldest first; returns the element count */
int env_state_screen(Env* e, void* out) {
    StatePacket state;
    e->g->get_state_data(0.0f, state);
    auto buf = state.get_buffer("screen");
    int n = (int)buf->get_value_size();
    if (buf->get_value()->is_uint8()) std::memcpy(out, buf->get_value<uint8_t>(), (size_t)n);
    else std::memcpy(out, buf->get_value<float>(), sizeof(float) * (size_t)n);
    return n;
}

int env_screen(Env* e, void* out) {
    StatePacket screen;
    e->g->get_screen(screen);
    auto buf = screen.get_buffer("screen");
    int n = (int)buf->get_value_size();
    if (buf->get_value()->is_uint8()) std::memcpy(out, buf->get_value<uint8_t>(), (size_t)n);
    else std::memcpy(out, buf->get_value<float>(), sizeof(float) * (size_t)n);
    return n;
}

void env_car(Env* e, float* out3) {
    if (e->game != 1) die("car state of a game that has no car");
    auto* r = static_cast<simulator::simple_race::SimpleRaceGame*>(e->g);
    cv::Point2f p = r->_race._car.get_pos();
    out3[0] = p.x;
    out3[1] = p.y;
    out3[2] = r->_race._car.get_angle();
}

}  // namespace

extern "C" {

void xwref_set_common_flags(int context, int max_steps, int simulator_seed) {
    FLAGS_context = context;
    FLAGS_max_steps = max_steps;
    FLAGS_simulator_seed = simulator_seed;
}

void xwref_set_game_flags(int array_size) { FLAGS_array_size = array_size; }

void xwref_set_race_flags(const char* track_type, double track_width, double track_length, double track_radius,
                          int race_full_manouver, int random, const char* difficulty, double reward_scale) {
    FLAGS_track_type = track_type;
    FLAGS_track_width = track_width;
    FLAGS_track_length = track_length;
    FLAGS_track_radius = track_radius;
    FLAGS_race_full_manouver = race_full_manouver != 0;
    FLAGS_random = random != 0;
    FLAGS_difficulty = difficulty;
    FLAGS_reward_scale = reward_scale;
}

/* threads the reference's counter has counted so far (see the header comment) */
int xwref_threads(void) { return g_threads; }

/* count n threads that make no env: each only constructs its engine */
void xwref_burn_threads(int n) {
    for (int i = 0; i < n; ++i) {
        std::thread th([] { (void)simulator::util::thread_local_reng(); });
        th.join();
        if (FLAGS_simulator_seed) g_threads++;
    }
}

/* ---- one env on the caller's thread ---- */
void* xwref_create(int game) {
    if (game == 1 && FLAGS_random) die("FLAGS_random draws from the thread's engine: use xwref_rollout");
    return env_create(game);
}
void  xwref_destroy(void* h) { Env* e = (Env*)h; delete e->g; delete e; }
void  xwref_reset_game(void* h) { env_reset((Env*)h); }
float xwref_take_actions(void* h, int action, int act_rep) { return env_take_actions((Env*)h, action, act_rep); }
int   xwref_game_over(void* h) { return ((Env*)h)->g->game_over(); }
int   xwref_get_num_actions(void* h) { return ((Env*)h)->g->get_num_actions(); }
int   xwref_get_lives(void* h) { return ((Env*)h)->g->get_lives(); }
long long xwref_get_num_steps(void* h) { return (long long)((Env*)h)->g->get_num_steps(); }
int   xwref_get_screen(void* h, void* out) { return env_screen((Env*)h, out); }
int   xwref_get_state_screen(void* h, void* out) { return env_state_screen((Env*)h, out); }
void  xwref_get_car(void* h, float* out3) { env_car((Env*)h, out3); }

/* ---- one env on a fresh thread: the example loop (examples/test_simple_race.cpp: game over? reset; state; act) ----
 * Construct (the constructor resets once), reset_game, then for t < steps: reset when game_over() != 0; record the state
 * screen [, the car] into obs / cars; take actions[t]; record reward, code, step count and the state screen [, the car]
 * right after the step into obs_after / cars_after.  One more "reset when over; record" closes the run, so obs / cars /
 * reset_flags hold steps + 1 records.  obs_stride is in bytes.  The car pointers may be NULL (SimpleGame). */
int xwref_rollout(int game, int steps, const int32_t* actions, float* rewards, uint8_t* codes, int32_t* num_steps,
                  void* obs, void* obs_after, int obs_stride, float* cars, float* cars_after, uint8_t* reset_flags,
                  float* ctor_car) {
    int n_actions = 0;
    std::thread th([&] {
        (void)simulator::util::thread_local_reng();
        Env* e = env_create(game);
        if (ctor_car) env_car(e, ctor_car);
        n_actions = e->g->get_num_actions();
        env_reset(e);
        for (int t = 0; t <= steps; ++t) {
            reset_flags[t] = 0;
            if (e->g->game_over() != 0) {
                env_reset(e);
                reset_flags[t] = 1;
            }
            env_state_screen(e, (char*)obs + (size_t)t * (size_t)obs_stride);
            if (cars) env_car(e, cars + 3 * t);
            if (t == steps) break;
            rewards[t] = env_take_actions(e, actions[t], 1);
            codes[t] = (uint8_t)e->g->game_over();
            num_steps[t] = (int32_t)e->g->get_num_steps();
            env_state_screen(e, (char*)obs_after + (size_t)t * (size_t)obs_stride);
            if (cars_after) env_car(e, cars_after + 3 * t);
        }
        delete e->g;
        delete e;
    });
    th.join();
    if (FLAGS_simulator_seed) g_threads++;
    return n_actions;
}

}  /* extern "C" */
