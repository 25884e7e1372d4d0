"""Writes tests/golden/expert_bfs.json: for random boards, the length of the path the reference's own breadth-first search
(python/maze2d.py: bfs, the search behind the teacher's _reachable) returns -- the cells strictly between start and end, so a
path of m moves has length m - 1 -- or null when the end cannot be reached.  Recorded results only; run by hand with the
reference's python directory as the argument:  python tests/golden/make_expert_golden.py <reference>/python"""
import json
import os
import random
import sys


def main():
    sys.path.insert(0, sys.argv[1])
    import maze2d
    rng = random.Random(20261016)
    boards = []
    for i in range(320):
        X, Y = rng.randint(3, 8), rng.randint(3, 8)
        cells = [(x, y) for y in range(Y) for x in range(X)]
        rng.shuffle(cells)
        start, end = cells[0], cells[1]
        obstacles = cells[2:2 + rng.randint(0, (X * Y) // 2)]
        random.seed(i)
        path = maze2d.bfs(start + (0,), end + (0,), X, Y, set(o + (0,) for o in obstacles))
        boards.append({"X": X, "Y": Y, "start": list(start), "end": list(end), "obstacles": [list(o) for o in sorted(obstacles)],
                       "length": None if path is None else len(path)})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "expert_bfs.json")
    with open(out, "w") as f:
        json.dump({"source": "python/maze2d.py bfs(start, end, X, Y, obstacles): len(result) or null", "boards": boards}, f,
                  separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
